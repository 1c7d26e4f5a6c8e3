// Host-side AddressSanitizer sweep of the convolution planner (tpg_plan_data.hip,
// tpg_plan_wgrad.hip) through the entry points of tpg_capi.hip.
//
// The planner (check_desc -> plan_data / plan_probs / maybe_halo / plan_bwd_filter ->
// workspace and pre-pack sizing) is pure host code: it runs before any launch and sizes the
// buffers every kernel later indexes, so an out-of-range tap table, a vector overrun or a
// wrong region size shows up here first.  This driver feeds it a deterministic sweep of
// valid geometries (TP-GAN's layer shapes plus a random walk over kernel / stride / pad /
// channel / dtype / transposed / flags combinations) and of malformed descriptors, through
// every entry point that does no device work:
//   tpg_conv2d_workspace (all three ops and out-of-range op codes),
//   tpg_conv2d_packed_bytes, tpg_conv2d_pack_jobs (host job table only), tpg_pack_prepare,
//   tpg_conv2d_wgrad_plan (the weight gradient's kernel / tile / pixel-split choice and
//   argument fill, on four tensor layouts per valid descriptor; the plan must be consistent),
//   tpg_conv2d_data_plan (the forward, input-gradient and masked input-gradient plans of every
//   valid descriptor on the same four layouts: kernel per problem, tiles, k splits, workspace
//   regions; consistent, and never short of the workspace tpg_conv2d_workspace reports),
//   and the launch entry points with descriptors check_desc rejects (validation path only).
// The LANCZOS resize's host side (tpg_resize.hip) is swept too: tpg_resize_ksize / _coeffs over a
// seeded sample of input sizes in 1..4096 times the outputs {1, 32, 64, 128, 256}, into heap
// arrays of exactly out*2 and out*ksize ints (an off-by-one in ksize writes past them), and the
// job builder and size queries with malformed arguments.
// The identity search's host side (tpg_identity.hip) too: tpg_cosine_topk_workspace over a seeded walk
// of (P, G, k, gchunk) up to 2^24 rows, whose size must be positive, hold at least one k-entry list
// per probe and chunk and not shrink when P or the number of chunks grows, and every argument the
// three launch entry points reject (which must stop them before any device work).
// The landmark front end's entry points (tpg_ssd_landmarks, tpg_landmark_accuracy, tpg_u8_to_unit)
// likewise: NULL pointers and sizes outside their ranges (n = 0 and 4097, C = 4, 0 and 9 bands, ...),
// with the host-read tables (patch sizes, band edges and weights, strides) in exact-size heap blocks.
// The face alignment's host side (tpg_align.hip) too: tpg_warp_pack_job into a heap block of exactly
// two records, tpg_similarity_fit's template check with the template in an exact-size heap block of
// K * 2 floats (non-finite, coincident and overflowing templates, K outside 2..8), and every argument
// tpg_similarity_fit and tpg_affine_warp_u8 reject, which must stop them before any device work.
// Built with `make -C tp-gan_amd asan` (the host-logic units compiled with -fsanitize=address on
// the host side only; the kernels are the product's) and run by tests/test_capi.py.
// Exit status: 0 clean, 1 a consistency check failed; ASan aborts on a memory error.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/tpgan.h"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 11);
}
static int pick(const int* v, int n) { return v[rnd() % n]; }

static int g_fail = 0;
static long g_valid = 0, g_rejected = 0, g_jobs = 0, g_plans = 0, g_dplans = 0;

// channels-last activation of a never-dereferenced buffer, in the layouts of
// tests/golden/make_wgrad_plans.py: 0 channels padded to 8, 1 as they are, 2 a view narrower
// than its buffer, 3 a batch stride of 2^30 elements (byte extent past 2^31)
static tpg_tensor fake_act(int c, int h, int w, int dtype, int layout) {
  tpg_tensor t;
  memset(&t, 0, sizeof(t));
  const int64_t cp = layout == 1 ? c : (c + 7) / 8 * 8, row = (w + (layout == 2 ? 2 : 0)) * cp;
  t.data = (void*)0x10000;
  t.dtype = dtype;
  t.stride[0] = h * row; t.stride[1] = 1; t.stride[2] = row; t.stride[3] = cp;
  if (layout == 3 && t.stride[0] < (1ll << 30)) t.stride[0] = 1ll << 30;
  return t;
}

// The weight-gradient plan of a valid descriptor (its own algo / ksplit / flags) in every
// layout: tile cost models, the pixel-split model, byte extents and the argument fill all run
// here, and the plan that comes back must be one a launch could use.
static void check_wgrad_plans(const tpg_conv_desc* d) {
  for (int layout = 0; layout < 4; ++layout) {
    const tpg_tensor x = fake_act(d->in_c, d->in_h, d->in_w, d->dtype, layout);
    const tpg_tensor g = fake_act(d->out_c, d->out_h, d->out_w, d->dtype, layout);
    const int b = d->transposed ? d->out_c : d->in_c;
    tpg_tensor dw = fake_act(b, d->kh, d->kw, TPG_F32, 1);
    tpg_wgrad_plan* p = (tpg_wgrad_plan*)malloc(sizeof(tpg_wgrad_plan));
    const int32_t rc = tpg_conv2d_wgrad_plan(d, x, g, dw, p);
    ++g_plans;
    const char* why = nullptr;
    if (rc == 0) {
      const bool halo = p->kernel == TPG_WGRAD_ROW_HALO || p->kernel == TPG_WGRAD_IMAGE_HALO;
      const int PH = d->transposed ? d->in_h : d->out_h, PW = d->transposed ? d->in_w : d->out_w;
      // what the splits must cover: pixels of the iteration grid (1 x 1 in the GEMM forms), or
      // the halo kernels' 64-pixel k-tiles of (64 / tw) rows of tw = min(width, 64) pixels
      const int tw = p->kernel == TPG_WGRAD_IMAGE_HALO && PW < 64 ? PW : 64;
      const int64_t need = halo ? (int64_t)d->n * ((PH + 64 / tw - 1) / (64 / tw)) * (PW / tw) : (int64_t)d->n * PH * PW;
      const int64_t have = (int64_t)p->per_split * p->splits;
      if (p->kernel < TPG_WGRAD_GENERIC || p->kernel > TPG_WGRAD_IMAGE_HALO) why = "kernel kind out of range";
      else if (p->splits < 1) why = "splits < 1";
      else if (p->tiles < 1) why = "tiles < 1";
      else if (p->tile_m < 1 || p->tile_n < 1) why = "empty tile";
      else if (have < need) why = "splits do not cover the pixels";
      else if (halo && (d->dtype == TPG_F32 || d->stride_h != 1 || d->stride_w != 1 || d->transposed))
        why = "halo kernel for an fp32, strided or transposed conv";
      else if (halo != (p->taps_per_block > 0)) why = "taps_per_block disagrees with the kernel kind";
    } else if (rc != -30 && rc != -4) {
      why = "unexpected status";
    }
    if (why) {
      fprintf(stderr, "wgrad plan (layout %d, rc %d): %s: n=%d c=%d->%d %dx%d->%dx%d k=%dx%d s=%d,%d T=%d dt=%d algo=%d ks=%d fl=%d: %s\n",
              layout, rc, why, d->n, d->in_c, d->out_c, d->in_h, d->in_w, d->out_h, d->out_w, d->kh, d->kw, d->stride_h,
              d->stride_w, d->transposed, d->dtype, d->algo, d->ksplit, d->flags, rc ? tpg_last_error() : "");
      g_fail = 1;
    }
    free(p);
  }
}

// The forward / input-gradient plans of a valid descriptor in every layout, offered the workspace
// the size query reports: a plan that comes back must be one the launch sequence could run.
static const char* data_plan_fault(const tpg_conv_desc* d, const tpg_data_plan* p, int op) {
  if (p->nprobs < 1 || p->nprobs > TPG_DATA_MAX_PROBS) return "problem count out of range";
  const bool packed = d->flags & TPG_FLAG_WPACKED;
  uint64_t end = packed ? 0 : p->tmp_bytes, sk = 0;
  for (int i = 0; i < p->nprobs; ++i) {
    const tpg_data_prob& q = p->prob[i];
    if (q.kernel < TPG_DATA_GENERIC || q.kernel > TPG_DATA_POINTWISE) return "kernel kind out of range";
    if (q.kernel == TPG_DATA_GENERIC) {
      if (q.cfg < 0 || q.cfg > 5 || q.bn < 1 || q.rows < 1) return "generic config out of range";
    } else {
      const bool c256 = q.cfg >= 0 && q.cfg < 24, c512 = q.cfg == 24 || q.cfg == 25;
      const bool s2 = (q.cfg >= 40 && q.cfg <= 43) || q.cfg == 47;
      if (!c256 && !c512 && !s2) return "halo config out of range";
      if (q.rows != (c512 ? 512 : 256)) return "rows disagree with the config";
      if (q.th < 1 || q.tw < 1 || q.img < 1 || (int64_t)q.th * q.tw * q.img > q.rows) return "tile larger than the block";
      if (q.halo_px < q.img || q.halo_px > (c256 ? (q.cfg / 8 + 3) * 128 : 1024)) return "halo past its class";
      if ((q.kernel == TPG_DATA_POINTWISE) != (q.pw_tile >= 1 && q.pw_tile <= 4)) return "pointwise tile disagrees";
    }
    if (q.taps > 0 && (q.ksplit < 1 || q.kps < 1 || (int64_t)q.ksplit * q.kps < q.ksteps ||
                       (int64_t)(q.ksplit - 1) * q.kps >= q.ksteps))
      return "k split does not cover the k-steps";
    if (q.wp_off < end) return "weight regions overlap";
    end = q.wp_off + q.wp_bytes;
    if (q.sk_bytes > sk) sk = q.sk_bytes;
  }
  if (end > (packed ? p->packed_bytes : p->ws_bytes)) return "weight regions end outside their buffer";
  if (p->sk_off < (packed ? p->tmp_bytes : end) || p->sk_off + sk > p->ws_bytes) return "split-K slices outside the workspace";
  if (((p->flags & TPG_DATA_REFLECT_FOLD) != 0) != (p->tmp_bytes > 0)) return "reflect temp disagrees with the form";
  if (p->flags & TPG_DATA_MASKED)
    if (op != TPG_OP_BWD_DATA_MASKED || p->nprobs != 1 || p->prob[0].kernel != TPG_DATA_HALO || p->prob[0].taps < 2)
      return "masked mode off a single multi-tap halo problem";
  if (op == TPG_OP_BWD_DATA_MASKED && !(p->flags & TPG_DATA_MASKED)) return "masked op without masked mode";
  return nullptr;
}

static void check_data_plans(const tpg_conv_desc* d0) {
  const int ops[3] = {TPG_OP_FWD, TPG_OP_BWD_DATA, TPG_OP_BWD_DATA_MASKED};
  for (int layout = 0; layout < 4; ++layout)
    for (int op : ops) {
      tpg_conv_desc* d = (tpg_conv_desc*)malloc(sizeof(tpg_conv_desc));
      memcpy(d, d0, sizeof(*d));
      if (op != TPG_OP_FWD && (layout & 1)) { d->in_act = TPG_ACT_LEAKY; d->in_slope = 0.2f; }
      const tpg_tensor x = fake_act(d->in_c, d->in_h, d->in_w, d->dtype, layout);
      const tpg_tensor y = fake_act(d->out_c, d->out_h, d->out_w, d->dtype, layout);
      tpg_data_plan* p = (tpg_data_plan*)malloc(sizeof(tpg_data_plan));
      const size_t ws = tpg_conv2d_workspace(d, op == TPG_OP_FWD ? TPG_OP_FWD : TPG_OP_BWD_DATA);
      const int32_t rc = op == TPG_OP_FWD ? tpg_conv2d_data_plan(d, op, x, y, y, y, x, ws, p)
                                          : tpg_conv2d_data_plan(d, op, y, x, y, y, x, ws, p);
      ++g_dplans;
      const char* why = nullptr;
      if (rc == 0) why = data_plan_fault(d, p, op);
      else if (rc != -4 && rc != -21 && rc != -32 && !(rc == -31 && op == TPG_OP_BWD_DATA_MASKED)) why = "unexpected status";
      if (why) {
        fprintf(stderr, "data plan (op %d, layout %d, rc %d): %s: n=%d c=%d->%d %dx%d->%dx%d k=%dx%d s=%d,%d T=%d dt=%d ks=%d algo=%d fl=%d: %s\n",
                op, layout, rc, why, d->n, d->in_c, d->out_c, d->in_h, d->in_w, d->out_h, d->out_w, d->kh, d->kw,
                d->stride_h, d->stride_w, d->transposed, d->dtype, d->data_ksplit, d->data_algo, d->flags,
                rc ? tpg_last_error() : "");
        g_fail = 1;
      }
      free(p);
      free(d);
    }
}

static void run_one(const tpg_conv_desc& d0, bool expect_valid) {
  // the descriptor is copied to a heap block of exactly its size so a read past it is caught
  tpg_conv_desc* d = (tpg_conv_desc*)malloc(sizeof(tpg_conv_desc));
  memcpy(d, &d0, sizeof(*d));
  size_t ws[3];
  for (int op = 0; op < 3; ++op) ws[op] = tpg_conv2d_workspace(d, op);
  (void)tpg_conv2d_workspace(d, -1);
  (void)tpg_conv2d_workspace(d, 3);
  const bool ok = ws[0] != 0;  // 0 = rejected by check_desc; a valid plan needs >= 256
  if (ok) ++g_valid; else ++g_rejected;
  if (expect_valid && !ok) {
    fprintf(stderr, "valid descriptor rejected: n=%d c=%d->%d %dx%d->%dx%d k=%dx%d s=%d pad=%d,%d,%d,%d T=%d dt=%d: %s\n",
            d->n, d->in_c, d->out_c, d->in_h, d->in_w, d->out_h, d->out_w, d->kh, d->kw, d->stride_h, d->pad_t,
            d->pad_b, d->pad_l, d->pad_r, d->transposed, d->dtype, tpg_last_error());
    g_fail = 1;
  }
  for (int op = 0; op < 3; ++op)
    if ((ws[op] != 0) != ok) { fprintf(stderr, "workspace(op=%d) disagrees with check_desc\n", op); g_fail = 1; }
  for (int op = 0; op < 2; ++op) {
    const size_t pb = tpg_conv2d_packed_bytes(d, op);
    if (ok && pb + 256 > ws[op] && !(d->flags & TPG_FLAG_WPACKED)) {
      // the pre-packed image is the weight part of the op's workspace
      fprintf(stderr, "packed_bytes(op=%d)=%zu exceeds workspace %zu\n", op, pb, ws[op]);
      g_fail = 1;
    }
    // host job table: an exact-size heap block, a short table, and a table of zero entries
    const size_t jb = tpg_pack_job_bytes();
    const int cap = 1 + (int)(rnd() % 8);
    void* jobs = malloc(jb * cap);
    std::vector<float> w(16, 0.f);
    tpg_tensor wt;
    memset(&wt, 0, sizeof(wt));
    wt.data = w.data();
    wt.dtype = TPG_F32;
    char* wp = (char*)0x10000;  // only offset, never dereferenced on the host
    const int n = tpg_conv2d_pack_jobs(d, op, wt, wp, jobs, cap);
    if (n > 0) {
      g_jobs += n;
      const int64_t nb = tpg_pack_prepare(jobs, n);
      if (nb <= 0) { fprintf(stderr, "pack_prepare returned %lld for %d jobs\n", (long long)nb, n); g_fail = 1; }
    }
    (void)tpg_conv2d_pack_jobs(d, op, wt, wp, jobs, 0);
    free(jobs);
  }
  if (ok) check_wgrad_plans(d);
  if (ok) check_data_plans(d);
  if (!ok) {  // launch entry points must stop at validation (no device work happens)
    tpg_tensor z;
    memset(&z, 0, sizeof(z));
    if (tpg_conv2d_fwd(d, z, z, nullptr, z, z, nullptr, 0, nullptr) == 0 ||
        tpg_conv2d_bwd_data(d, z, z, z, nullptr, 0, nullptr) == 0 ||
        tpg_conv2d_bwd_filter(d, z, z, z, nullptr, 0, nullptr) == 0) {
      fprintf(stderr, "launch entry accepted a rejected descriptor\n");
      g_fail = 1;
    }
  }
  free(d);
}

// Resize tables: every window must lie inside the axis and the table row, the weights of a row
// must sum to 1.0 in 22 fractional bits up to the rounding of its taps, and the tail is zero.
static long g_tables = 0;
static void resize_table(int in, int out) {
  const int ks = tpg_resize_ksize(in, out);
  const double scale = (double)in / out, sup = 3.0 * (scale < 1.0 ? 1.0 : scale);
  int want = (int)sup;
  if (want < sup) ++want;
  want = want * 2 + 1;
  if (ks != want || tpg_resize_table_ints(in, out) != (int64_t)out * (2 + ks)) {
    fprintf(stderr, "resize_ksize(%d, %d) = %d, expected %d\n", in, out, ks, want);
    g_fail = 1;
    return;
  }
  int32_t* bounds = (int32_t*)malloc(sizeof(int32_t) * 2 * out);
  int32_t* k = (int32_t*)malloc(sizeof(int32_t) * (size_t)out * ks);
  if (tpg_resize_coeffs(in, out, bounds, k) != 0) {
    fprintf(stderr, "resize_coeffs(%d, %d): %s\n", in, out, tpg_last_error());
    g_fail = 1;
  } else {
    for (int xx = 0; xx < out; ++xx) {
      const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
      int64_t sum = 0;
      for (int x = 0; x < ks; ++x) {
        if (x >= n && k[(size_t)xx * ks + x] != 0) {
          fprintf(stderr, "resize %d->%d: tail not zero\n", in, out);
          g_fail = 1;
        }
        sum += k[(size_t)xx * ks + x];
      }
      if (xmin < 0 || n < 1 || n > ks || xmin + n > in || sum < (1 << 22) - n || sum > (1 << 22) + n) {
        fprintf(stderr, "resize %d->%d row %d: xmin %d n %d sum %lld\n", in, out, xx, xmin, n, (long long)sum);
        g_fail = 1;
      }
    }
  }
  free(bounds);
  free(k);
  ++g_tables;
}

static void resize_jobs() {
  const size_t jb = tpg_resize_job_bytes();
  char* jobs = (char*)malloc(jb * 2);  // records 0 and 1, nothing after them
  const uint8_t* src = (const uint8_t*)0x10000;  // recorded, never dereferenced on the host
  const int bad[] = {0, -1, 4097, -2147483647 - 1, 2147483647};
  if (tpg_resize_pack_job(jobs, 0, src, 480, 640, 3, 1920, 128, 128, 0, 4224, 0) != 0 ||
      tpg_resize_pack_job(jobs, 1, src, 4096, 4096, 3, 12288, 1, 4096, 0, 0, 16) != 0 ||
      tpg_resize_workspace(480, 640, 128, 128) != 480 * 128 * 3 ||
      tpg_resize_workspace(128, 640, 128, 128) != 0) {
    fprintf(stderr, "resize job builder rejected a valid job: %s\n", tpg_last_error());
    g_fail = 1;
  }
  int accepted = 0;
  for (int v : bad) {
    accepted += tpg_resize_pack_job(jobs, 1, src, v, 640, 3, 1920, 128, 128, 0, 0, 0) == 0;
    accepted += tpg_resize_pack_job(jobs, 1, src, 480, v, 3, 12288, 128, 128, 0, 0, 0) == 0;
    accepted += tpg_resize_pack_job(jobs, 1, src, 480, 640, 3, 1920, v, 128, 0, 0, 0) == 0;
    accepted += tpg_resize_pack_job(jobs, 1, src, 480, 640, 3, 1920, 128, v, 0, 0, 0) == 0;
    accepted += tpg_resize_pack_job(jobs, 1, src, 480, 640, v, 1920, 128, 128, 0, 0, 0) == 0;
    accepted += tpg_resize_pack_job(jobs, 1, src, 480, 640, 3, v < 1920 ? v : 1919, 128, 128, 0, 0, 0) == 0;
    accepted += tpg_resize_workspace(v, 640, 128, 128) >= 0;
    accepted += tpg_resize_workspace(480, 640, 128, v) >= 0;
    accepted += tpg_resize_ksize(v, 128) != 0;
    accepted += tpg_resize_ksize(128, v) != 0;
    accepted += tpg_resize_table_ints(v, v) != 0;
    accepted += tpg_resize_coeffs(v, 128, (int32_t*)jobs, (int32_t*)jobs) == 0;
    accepted += tpg_resize_coeffs(128, v, (int32_t*)jobs, (int32_t*)jobs) == 0;
  }
  accepted += tpg_resize_pack_job(jobs, -1, src, 480, 640, 3, 1920, 128, 128, 0, 0, 0) == 0;
  accepted += tpg_resize_pack_job(jobs, 1, nullptr, 480, 640, 3, 1920, 128, 128, 0, 0, 0) == 0;
  accepted += tpg_resize_pack_job(nullptr, 1, src, 480, 640, 3, 1920, 128, 128, 0, 0, 0) == 0;
  accepted += tpg_resize_pack_job(jobs, 1, src, 480, 640, 3, 1920, 128, 128, -4, 0, 0) == 0;
  accepted += tpg_resize_pack_job(jobs, 1, src, 480, 640, 3, 1920, 128, 128, 0, 0, 24) == 0;
  accepted += tpg_resize_coeffs(64, 32, nullptr, nullptr) == 0;
  accepted += tpg_resize_u8(1, nullptr, nullptr, 128, 128, nullptr, nullptr, nullptr) == 0;
  accepted += tpg_resize_u8(-1, jobs, (const int32_t*)jobs, 128, 128, (uint8_t*)jobs, nullptr, nullptr) == 0;
  if (accepted) { fprintf(stderr, "resize: %d malformed calls accepted\n", accepted); g_fail = 1; }
  free(jobs);
}

// Face alignment: the job builder and the two launch entry points' validation.  Every launch call is
// malformed in exactly one way; device pointers are fake and never dereferenced on the host.
static void align_sweep() {
  const size_t jb = tpg_warp_job_bytes();
  char* jobs = (char*)malloc(jb * 2);  // records 0 and 1, nothing after them
  const uint8_t* src = (const uint8_t*)0x10000;
  void* devp = (void*)0x20000;
  const int bad[] = {0, -1, 4097, -2147483647 - 1, 2147483647};
  if (jb != 32 || tpg_warp_pack_job(jobs, 0, src, 480, 640, 3, 1920, 128, 128) != 0 ||
      tpg_warp_pack_job(jobs, 1, src, 4096, 4096, 3, 12288 + 64, 1, 4096) != 0) {
    fprintf(stderr, "warp job builder rejected a valid job: %s\n", tpg_last_error());
    g_fail = 1;
  }
  int accepted = 0;
  for (int v : bad) {
    accepted += tpg_warp_pack_job(jobs, 1, src, v, 640, 3, 1920, 128, 128) == 0;
    accepted += tpg_warp_pack_job(jobs, 1, src, 480, v, 3, 12288, 128, 128) == 0;
    accepted += tpg_warp_pack_job(jobs, 1, src, 480, 640, 3, 1920, v, 128) == 0;
    accepted += tpg_warp_pack_job(jobs, 1, src, 480, 640, 3, 1920, 128, v) == 0;
    accepted += tpg_warp_pack_job(jobs, 1, src, 480, 640, v, 1920, 128, 128) == 0;
    accepted += tpg_warp_pack_job(jobs, 1, src, 480, 640, 3, v < 1920 ? v : 1919, 128, 128) == 0;
    accepted += tpg_affine_warp_u8(1, devp, (const int32_t*)devp, v, 128, (uint8_t*)devp, (int32_t*)devp, nullptr) == 0;
    accepted += tpg_affine_warp_u8(1, devp, (const int32_t*)devp, 128, v, (uint8_t*)devp, (int32_t*)devp, nullptr) == 0;
  }
  accepted += tpg_warp_pack_job(jobs, -1, src, 480, 640, 3, 1920, 128, 128) == 0;
  accepted += tpg_warp_pack_job(jobs, 1, nullptr, 480, 640, 3, 1920, 128, 128) == 0;
  accepted += tpg_warp_pack_job(nullptr, 1, src, 480, 640, 3, 1920, 128, 128) == 0;
  accepted += tpg_affine_warp_u8(-1, devp, (const int32_t*)devp, 128, 128, (uint8_t*)devp, (int32_t*)devp, nullptr) == 0;
  accepted += tpg_affine_warp_u8(65536, devp, (const int32_t*)devp, 128, 128, (uint8_t*)devp, (int32_t*)devp, nullptr) == 0;
  accepted += tpg_affine_warp_u8(1, nullptr, (const int32_t*)devp, 128, 128, (uint8_t*)devp, (int32_t*)devp, nullptr) == 0;
  accepted += tpg_affine_warp_u8(1, devp, nullptr, 128, 128, (uint8_t*)devp, (int32_t*)devp, nullptr) == 0;
  accepted += tpg_affine_warp_u8(1, devp, (const int32_t*)devp, 128, 128, nullptr, (int32_t*)devp, nullptr) == 0;
  accepted += tpg_affine_warp_u8(1, devp, (const int32_t*)devp, 128, 128, (uint8_t*)devp, nullptr, nullptr) == 0;
  free(jobs);
  float* fd = (float*)devp;
  int32_t* id = (int32_t*)devp;
  for (int K = 2; K <= 8; ++K) {
    float* t = (float*)malloc(sizeof(float) * 2 * K);  // exactly K points: the check reads no further
    for (int k = 0; k < 2 * K; ++k) t[k] = 7.0f;       // coincident
    accepted += tpg_similarity_fit(4, K, fd, t, nullptr, fd, id, id, nullptr) == 0;
    for (int k = 0; k < 2 * K; ++k) t[k] = (float)(k * k % 11);
    t[2 * K - 1] = __builtin_nanf("");
    accepted += tpg_similarity_fit(4, K, fd, t, nullptr, fd, id, id, nullptr) == 0;
    t[2 * K - 1] = __builtin_inff();
    accepted += tpg_similarity_fit(4, K, fd, t, nullptr, fd, id, id, nullptr) == 0;
    t[2 * K - 1] = 3.0e38f;
    t[0] = -3.0e38f;  // finite points whose spread overflows float32
    accepted += tpg_similarity_fit(4, K, fd, t, nullptr, fd, id, id, nullptr) == 0;
    t[2 * K - 1] = 5.0f;
    t[0] = 1.0f;  // a good template: each missing pointer alone
    accepted += tpg_similarity_fit(4, K, nullptr, t, nullptr, fd, id, id, nullptr) == 0;
    accepted += tpg_similarity_fit(4, K, fd, t, nullptr, nullptr, id, id, nullptr) == 0;
    accepted += tpg_similarity_fit(4, K, fd, t, nullptr, fd, nullptr, id, nullptr) == 0;
    accepted += tpg_similarity_fit(4, K, fd, t, nullptr, fd, id, nullptr, nullptr) == 0;
    accepted += tpg_similarity_fit(-1, K, fd, t, nullptr, fd, id, id, nullptr) == 0;
    free(t);
  }
  float two[4] = {0, 0, 1, 1};
  for (int K : {-1, 0, 1, 9, 2147483647}) accepted += tpg_similarity_fit(4, K, fd, two, nullptr, fd, id, id, nullptr) == 0;
  accepted += tpg_similarity_fit(4, 2, fd, nullptr, nullptr, fd, id, id, nullptr) == 0;
  if (accepted) { fprintf(stderr, "align: %d malformed calls accepted\n", accepted); g_fail = 1; }
}

// Identity search: the chunk planner and the validation of tpg_l2_normalize / tpg_cosine_topk /
// tpg_cosine_pairs.  Every launch call below is malformed in exactly one way; the pointers are never
// dereferenced on the host.
static long g_idplans = 0;
static void identity_sweep(long iters) {
  const int ks[] = {1, 2, 5, 8}, bad_k[] = {0, -1, 9, 2147483647}, bad_chunk[] = {1, 7, 15, -1, -2147483647 - 1};
  const int sizes[] = {0, 1, 2, 17, 64, 127, 128, 129, 300, 1031, 4096, 16384, 131072, 1 << 20, (1 << 24) - 1, 1 << 24};
  for (long it = 0; it < iters; ++it) {
    const int P = rnd() % 3 ? pick(sizes, 16) : (int)(rnd() % ((1u << 24) + 1));
    const int G = rnd() % 3 ? pick(sizes, 16) : (int)(rnd() % ((1u << 24) + 1));
    const int k = pick(ks, 4);
    int gchunk = rnd() % 2 ? 0 : 16 + (int)(rnd() % 5000);
    if (rnd() % 16 == 0) gchunk = 2147483647;
    const int64_t ws = tpg_cosine_topk_workspace(P, G, k, gchunk);
    ++g_idplans;
    if (ws < 0) {
      // only a forced chunk this small on a gallery this large may be refused (2^31 blocks)
      if (gchunk == 0 || ((int64_t)P + 127) / 128 * (((int64_t)G + gchunk - 1) / gchunk) <= 0x7fffffffLL) {
        fprintf(stderr, "cosine_topk_workspace(%d, %d, %d, %d) = %lld: %s\n", P, G, k, gchunk, (long long)ws, tpg_last_error());
        g_fail = 1;
      }
      continue;
    }
    int64_t least = gchunk ? (int64_t)8 * P * k * (((int64_t)G + gchunk - 1) / gchunk) : (int64_t)8 * P * k * (G > 0);
    if (ws < 8 || ws < least) {
      fprintf(stderr, "cosine_topk_workspace(%d, %d, %d, %d) = %lld < %lld\n", P, G, k, gchunk, (long long)ws, (long long)least);
      g_fail = 1;
    }
    if (P < (1 << 24) && tpg_cosine_topk_workspace(P + 1, G, k, gchunk) < ws && tpg_cosine_topk_workspace(P + 1, G, k, gchunk) >= 0 && gchunk) {
      fprintf(stderr, "cosine_topk_workspace shrinks from P = %d to %d (G %d k %d gchunk %d)\n", P, P + 1, G, k, gchunk);
      g_fail = 1;
    }
    if (gchunk >= 32 && gchunk < 2147483647) {  // half the chunk length: at least as many chunks
      const int64_t w2 = tpg_cosine_topk_workspace(P, G, k, gchunk / 2);
      if (w2 >= 0 && w2 < ws) {
        fprintf(stderr, "cosine_topk_workspace shrinks with more chunks (P %d G %d k %d gchunk %d)\n", P, G, k, gchunk);
        g_fail = 1;
      }
    }
  }
  int accepted = 0;
  float* f = (float*)0x10000;
  int32_t* i32 = (int32_t*)0x20000;
  void* ws = (void*)0x30000;
  tpg_tensor t, nul;
  memset(&t, 0, sizeof(t));
  memset(&nul, 0, sizeof(nul));
  t.data = f; t.dtype = TPG_F32; t.stride[0] = 512; t.stride[1] = 1;
  nul.stride[0] = 512; nul.stride[1] = 1;
  tpg_tensor badt = t;
  badt.dtype = 7;
  for (int k : bad_k) {
    accepted += tpg_cosine_topk_workspace(4, 100, k, 0) >= 0;
    accepted += tpg_cosine_topk(4, 100, 512, 512, f, f, k, nullptr, 0, i32, f, ws, 1 << 20, nullptr) == 0;
  }
  for (int c : bad_chunk) {
    accepted += tpg_cosine_topk_workspace(4, 100, 1, c) >= 0;
    accepted += tpg_cosine_topk(4, 100, 512, 512, f, f, 1, nullptr, c, i32, f, ws, 1 << 20, nullptr) == 0;
  }
  const int bad_n[] = {-1, (1 << 24) + 1, -2147483647 - 1, 2147483647}, bad_d[] = {0, -1, 4097, 2147483647, -2147483647 - 1};
  for (int n : bad_n) {
    accepted += tpg_cosine_topk_workspace(n, 100, 1, 0) >= 0;
    accepted += tpg_cosine_topk_workspace(4, n, 1, 0) >= 0;
    accepted += tpg_cosine_topk(n, 100, 512, 512, f, f, 1, nullptr, 0, i32, f, ws, 1 << 20, nullptr) == 0;
    accepted += tpg_cosine_topk(4, n, 512, 512, f, f, 1, nullptr, 0, i32, f, ws, 1 << 20, nullptr) == 0;
    accepted += tpg_l2_normalize(n, 512, t, f, 512, f, i32, nullptr) == 0;
    accepted += tpg_cosine_pairs(n, 512, t, t, f, i32, nullptr) == 0;
  }
  for (int d : bad_d) {
    accepted += tpg_cosine_topk(4, 100, d, 512, f, f, 1, nullptr, 0, i32, f, ws, 1 << 20, nullptr) == 0;
    accepted += tpg_l2_normalize(4, d, t, f, 512, f, i32, nullptr) == 0;
    accepted += tpg_cosine_pairs(4, d, t, t, f, i32, nullptr) == 0;
  }
  // dpad that is not d rounded up to a multiple of 4
  accepted += tpg_l2_normalize(4, 515, t, f, 515, f, i32, nullptr) == 0;
  accepted += tpg_l2_normalize(4, 515, t, f, 520, f, i32, nullptr) == 0;
  accepted += tpg_l2_normalize(4, 512, t, f, 516, f, i32, nullptr) == 0;
  accepted += tpg_cosine_topk(4, 100, 515, 515, f, f, 1, nullptr, 0, i32, f, ws, 1 << 20, nullptr) == 0;
  accepted += tpg_cosine_topk(4, 100, 3, 8, f, f, 1, nullptr, 0, i32, f, ws, 1 << 20, nullptr) == 0;
  // NULL pointers, bad dtypes, misaligned rows, a short workspace
  accepted += tpg_l2_normalize(4, 512, nul, f, 512, f, i32, nullptr) == 0;
  accepted += tpg_l2_normalize(4, 512, t, nullptr, 512, f, i32, nullptr) == 0;
  accepted += tpg_l2_normalize(4, 512, t, f, 512, f, nullptr, nullptr) == 0;
  accepted += tpg_l2_normalize(4, 512, badt, f, 512, f, i32, nullptr) == 0;
  accepted += tpg_cosine_pairs(4, 512, nul, t, f, i32, nullptr) == 0;
  accepted += tpg_cosine_pairs(4, 512, t, nul, f, i32, nullptr) == 0;
  accepted += tpg_cosine_pairs(4, 512, t, t, nullptr, i32, nullptr) == 0;
  accepted += tpg_cosine_pairs(4, 512, t, t, f, nullptr, nullptr) == 0;
  accepted += tpg_cosine_pairs(4, 512, t, badt, f, i32, nullptr) == 0;
  accepted += tpg_cosine_topk(4, 100, 512, 512, nullptr, f, 1, nullptr, 0, i32, f, ws, 1 << 20, nullptr) == 0;
  accepted += tpg_cosine_topk(4, 100, 512, 512, f, nullptr, 1, nullptr, 0, i32, f, ws, 1 << 20, nullptr) == 0;
  accepted += tpg_cosine_topk(4, 100, 512, 512, f, f, 1, nullptr, 0, nullptr, f, ws, 1 << 20, nullptr) == 0;
  accepted += tpg_cosine_topk(4, 100, 512, 512, f, f, 1, nullptr, 0, i32, nullptr, ws, 1 << 20, nullptr) == 0;
  accepted += tpg_cosine_topk(4, 100, 512, 512, f, f, 1, nullptr, 0, i32, f, nullptr, 1 << 20, nullptr) == 0;
  accepted += tpg_cosine_topk(4, 100, 512, 512, f + 1, f, 1, nullptr, 0, i32, f, ws, 1 << 20, nullptr) == 0;
  accepted += tpg_cosine_topk(4, 100, 512, 512, f, f + 2, 1, nullptr, 0, i32, f, ws, 1 << 20, nullptr) == 0;
  accepted += tpg_cosine_topk(4, 100, 512, 512, f, f, 1, nullptr, 0, i32, f, (char*)ws + 4, 1 << 20, nullptr) == 0;
  const int64_t need = tpg_cosine_topk_workspace(4, 100, 8, 16);
  accepted += tpg_cosine_topk(4, 100, 512, 512, f, f, 8, nullptr, 16, i32, f, ws, (size_t)need - 1, nullptr) == 0;
  accepted += tpg_cosine_topk(4, 100, 512, 512, f, f, 8, nullptr, 16, i32, f, ws, 0, nullptr) == 0;
  if (need != 8 * 4 * 8 * 7) { fprintf(stderr, "cosine_topk_workspace(4, 100, 8, 16) = %lld\n", (long long)need); g_fail = 1; }
  if (accepted) { fprintf(stderr, "identity: %d malformed calls accepted\n", accepted); g_fail = 1; }
}

// Landmark front end: tpg_ssd_landmarks, tpg_landmark_accuracy and tpg_u8_to_unit must refuse every
// malformed call below before any device work, -2 for sizes and -10 for NULL pointers.  The device
// pointers are never dereferenced on the host; the HOST arrays are heap blocks of exactly their size.
static void landmark_sweep() {
  int wrong = 0;
  float* f = (float*)0x10000;
  int32_t* i32 = (int32_t*)0x20000;
  uint8_t* u8 = (uint8_t*)0x30000;
  int32_t* wh = (int32_t*)malloc(sizeof(int32_t) * 8);
  const int32_t wh0[8] = {40, 40, 40, 40, 40, 32, 48, 32};
  memcpy(wh, wh0, sizeof(wh0));
  const struct { int B, n, C; } bad_ssd[] = {{0, 394, 5}, {-1, 394, 5}, {2, 0, 5}, {2, 4097, 5}, {2, -1, 5},
                                             {2, 394, 4}, {2, 394, 0}, {2, 2147483647, 5}, {2, 394, -2147483647 - 1}};
  for (const auto& s : bad_ssd)
    wrong += tpg_ssd_landmarks(s.B, s.n, s.C, f, f, 0.5f, nullptr, wh, f, f, i32, i32, i32, nullptr) != -2;
  wrong += tpg_ssd_landmarks(2, 394, 5, nullptr, f, 0.5f, nullptr, wh, f, f, i32, i32, i32, nullptr) != -10;
  wrong += tpg_ssd_landmarks(2, 394, 5, f, nullptr, 0.5f, nullptr, wh, f, f, i32, i32, i32, nullptr) != -10;
  wrong += tpg_ssd_landmarks(2, 394, 5, f, f, 0.5f, nullptr, nullptr, f, f, i32, i32, i32, nullptr) != -10;
  wrong += tpg_ssd_landmarks(2, 394, 5, f, f, 0.5f, nullptr, wh, nullptr, f, i32, i32, i32, nullptr) != -10;
  wrong += tpg_ssd_landmarks(2, 394, 5, f, f, 0.5f, nullptr, wh, f, nullptr, i32, i32, i32, nullptr) != -10;
  wrong += tpg_ssd_landmarks(2, 394, 5, f, f, 0.5f, nullptr, wh, f, f, nullptr, i32, i32, nullptr) != -10;
  wrong += tpg_ssd_landmarks(2, 394, 5, f, f, 0.5f, nullptr, wh, f, f, i32, nullptr, i32, nullptr) != -10;
  wrong += tpg_ssd_landmarks(2, 394, 5, f, f, 0.5f, nullptr, wh, f, f, i32, i32, nullptr, nullptr) != -10;
  wrong += tpg_ssd_landmarks(2, 394, 5, (float*)((char*)f + 2), f, 0.5f, nullptr, wh, f, f, i32, i32, i32, nullptr) == 0;
  for (int k = 0; k < 8; ++k) {  // a patch side of zero or below
    wh[k] = k % 2 ? 0 : -40;
    wrong += tpg_ssd_landmarks(2, 394, 5, f, f, 0.5f, f, wh, f, f, i32, i32, i32, nullptr) != -2;
    wh[k] = wh0[k];
  }
  free(wh);
  for (int nb = 1; nb <= TPG_LM_MAX_BANDS; ++nb) {  // exact-size band tables, every valid count; B is bad
    float* thr = (float*)malloc(sizeof(float) * nb);
    float* wgt = (float*)malloc(sizeof(float) * nb);
    for (int i = 0; i < nb; ++i) { thr[i] = 5.f * (i + 1); wgt[i] = 1.f / (i + 1); }
    wrong += tpg_landmark_accuracy(0, f, f, nullptr, nb, thr, wgt, f, nullptr) != -2;
    wrong += tpg_landmark_accuracy(-3, f, f, i32, nb, thr, wgt, f, nullptr) != -2;
    wrong += tpg_landmark_accuracy(4, nullptr, f, nullptr, nb, thr, wgt, f, nullptr) != -10;
    wrong += tpg_landmark_accuracy(4, f, nullptr, nullptr, nb, thr, wgt, f, nullptr) != -10;
    wrong += tpg_landmark_accuracy(4, f, f, nullptr, nb, nullptr, wgt, f, nullptr) != -10;
    wrong += tpg_landmark_accuracy(4, f, f, nullptr, nb, thr, nullptr, f, nullptr) != -10;
    wrong += tpg_landmark_accuracy(4, f, f, nullptr, nb, thr, wgt, nullptr, nullptr) != -10;
    if (nb > 1) {  // descending, and a NaN edge
      thr[nb - 1] = thr[0] - 1.f;
      wrong += tpg_landmark_accuracy(4, f, f, nullptr, nb, thr, wgt, f, nullptr) != -2;
      thr[nb - 1] = __builtin_nanf("");
      wrong += tpg_landmark_accuracy(4, f, f, nullptr, nb, thr, wgt, f, nullptr) != -2;
    }
    thr[0] = -1.f;  // below the implied lower edge 0
    wrong += tpg_landmark_accuracy(4, f, f, nullptr, nb, thr, wgt, f, nullptr) != -2;
    // a band count outside 1..8 is refused before either table is read
    const int bad_nb[] = {0, 9, -1, 2147483647, -2147483647 - 1};
    for (int b : bad_nb) wrong += tpg_landmark_accuracy(4, f, f, nullptr, b, thr, wgt, f, nullptr) != -2;
    free(thr);
    free(wgt);
  }
  tpg_tensor out, nul, badt;
  memset(&out, 0, sizeof(out));
  out.data = f; out.dtype = TPG_BF16;
  out.stride[0] = 128 * 128 * 8; out.stride[1] = 1; out.stride[2] = 128 * 8; out.stride[3] = 8;
  nul = out; nul.data = nullptr;
  badt = out; badt.dtype = 5;
  int64_t* is = (int64_t*)malloc(sizeof(int64_t) * 4);
  is[0] = 128 * 128 * 3; is[1] = 1; is[2] = 128 * 3; is[3] = 3;
  const int bad_dim[] = {0, -1, -2147483647 - 1};
  for (int v : bad_dim) {
    wrong += tpg_u8_to_unit(v, 3, 128, 128, u8, is, out, nullptr) != -2;
    wrong += tpg_u8_to_unit(2, v, 128, 128, u8, is, out, nullptr) != -2;
    wrong += tpg_u8_to_unit(2, 3, v, 128, u8, is, out, nullptr) != -2;
    wrong += tpg_u8_to_unit(2, 3, 128, v, u8, is, out, nullptr) != -2;
  }
  wrong += tpg_u8_to_unit(32768, 3, 256, 256, u8, is, out, nullptr) != -2;  // 2^31 pixels
  wrong += tpg_u8_to_unit(2147483647, 3, 2147483647, 2147483647, u8, is, out, nullptr) != -2;
  wrong += tpg_u8_to_unit(2, 3, 128, 128, nullptr, is, out, nullptr) != -10;
  wrong += tpg_u8_to_unit(2, 3, 128, 128, u8, nullptr, out, nullptr) != -10;
  wrong += tpg_u8_to_unit(2, 3, 128, 128, u8, is, nul, nullptr) != -10;
  wrong += tpg_u8_to_unit(2, 3, 128, 128, u8, is, badt, nullptr) == 0;
  free(is);
  if (wrong) { fprintf(stderr, "landmark front end: %d malformed calls not refused as documented\n", wrong); g_fail = 1; }
}

static tpg_conv_desc conv(int n, int ci, int h, int w, int co, int k, int s, int p, int dt, bool T = false,
                          int op_pad = 0, int pm = TPG_PAD_ZERO) {
  tpg_conv_desc d;
  memset(&d, 0, sizeof(d));
  d.n = n; d.in_c = ci; d.in_h = h; d.in_w = w; d.out_c = co;
  d.kh = d.kw = k; d.stride_h = d.stride_w = s;
  d.pad_t = d.pad_b = d.pad_l = d.pad_r = p;
  d.pad_mode = pm; d.transposed = T ? 1 : 0; d.dtype = dt;
  d.slope = 0.2f; d.res_scale = 1.f;
  if (T) {
    d.out_h = (h - 1) * s - 2 * p + k + op_pad;
    d.out_w = (w - 1) * s - 2 * p + k + op_pad;
  } else {
    d.out_h = (h + 2 * p - k) / s + 1;
    d.out_w = (w + 2 * p - k) / s + 1;
  }
  return d;
}

int main(int argc, char** argv) {
  const long iters = argc > 1 ? atol(argv[1]) : 4000;
  const int dts[3] = {TPG_F32, TPG_BF16, TPG_F16};
  // TP-GAN's own layer shapes (global generator, local pathways, discriminator) at 128x128
  // and bs32, every dtype, plus the full-kernel GEMM forms (fc1, deconv from a 1x1 map)
  for (int dt : dts) {
    const int B = 32;
    run_one(conv(B, 3, 128, 128, 64, 7, 1, 3, dt), true);
    run_one(conv(B, 64, 128, 128, 64, 5, 2, 2, dt), true);
    run_one(conv(B, 64, 64, 64, 128, 3, 2, 1, dt), true);
    run_one(conv(B, 128, 32, 32, 256, 3, 2, 1, dt), true);
    run_one(conv(B, 256, 16, 16, 512, 3, 2, 1, dt), true);
    run_one(conv(B, 512, 8, 8, 512, 3, 1, 1, dt), true);
    run_one(conv(B, 64, 128, 128, 64, 3, 1, 1, dt, false, 0, TPG_PAD_REFLECT), true);
    run_one(conv(B, 64, 1, 1, 64, 8, 1, 0, dt, true), true);
    run_one(conv(B, 512, 8, 8, 256, 3, 2, 1, dt, true, 1), true);
    run_one(conv(B, 256, 16, 16, 128, 3, 2, 1, dt, true, 1), true);
    run_one(conv(B, 128, 32, 32, 64, 3, 2, 1, dt, true, 1), true);
    run_one(conv(B, 96, 128, 128, 64, 5, 1, 2, dt), true);
    run_one(conv(B, 64, 128, 128, 3, 3, 1, 1, dt), true);
    run_one(conv(B, 3, 40, 48, 64, 3, 1, 1, dt), true);
    run_one(conv(B, 64, 20, 24, 128, 3, 2, 1, dt), true);
    run_one(conv(B, 128, 10, 12, 64, 3, 2, 1, dt, true, 1), true);
    run_one(conv(B, 256, 16, 16, 1, 16, 1, 0, dt), true);  // a full-kernel GEMM form
  }
  const int chans[] = {1, 2, 3, 4, 7, 8, 12, 16, 32, 48, 64, 96, 128, 192, 256, 320, 512};
  const int sizes[] = {1, 2, 3, 4, 5, 7, 8, 10, 12, 16, 20, 24, 31, 32, 40, 48, 64, 96, 128, 256};
  const int batches[] = {1, 2, 3, 4, 8, 16, 32};
  for (long it = 0; it < iters; ++it) {
    tpg_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.n = pick(batches, 7);
    d.in_c = pick(chans, 17);
    d.out_c = pick(chans, 17);
    d.in_h = pick(sizes, 20);
    d.in_w = rnd() % 4 ? d.in_h : pick(sizes, 20);
    d.kh = 1 + rnd() % 7;
    d.kw = rnd() % 4 ? d.kh : 1 + rnd() % 7;
    if (rnd() % 40 == 0) d.kh = d.kw = 8 + rnd() % 9;  // large kernels: GEMM form or rejected
    d.stride_h = 1 + rnd() % 4;
    d.stride_w = rnd() % 4 ? d.stride_h : 1 + rnd() % 4;
    d.transposed = rnd() % 4 == 0;
    d.dtype = pick(dts, 3);
    d.pad_t = rnd() % d.kh; d.pad_b = rnd() % 3 ? d.pad_t : rnd() % d.kh;
    d.pad_l = rnd() % d.kw; d.pad_r = rnd() % 3 ? d.pad_l : rnd() % d.kw;
    d.pad_mode = (!d.transposed && rnd() % 5 == 0) ? TPG_PAD_REFLECT : TPG_PAD_ZERO;
    d.act = rnd() % 4; d.slope = 0.2f; d.res_scale = 1.f;
    d.ksplit = rnd() % 3 ? 0 : 1 + rnd() % 16;
    d.data_ksplit = rnd() % 3 ? 0 : 1 + rnd() % 64;
    d.data_algo = rnd() % 3 ? 0 : (int)(rnd() % 4) - 1;
    d.algo = rnd() % 3 ? 0 : (int)(rnd() % 15) - 1;
    d.flags = rnd() % 8;
    if (d.transposed) {
      d.out_h = (d.in_h - 1) * d.stride_h - d.pad_t - d.pad_b + d.kh + (int)(rnd() % d.stride_h);
      d.out_w = (d.in_w - 1) * d.stride_w - d.pad_l - d.pad_r + d.kw + (int)(rnd() % d.stride_w);
    } else {
      d.out_h = (d.in_h + d.pad_t + d.pad_b - d.kh) / d.stride_h + 1;
      d.out_w = (d.in_w + d.pad_l + d.pad_r - d.kw) / d.stride_w + 1;
    }
    // geometries with an empty output or padding the reflect rule forbids are expected to be
    // rejected; everything else must plan
    bool valid = d.out_h > 0 && d.out_w > 0 && (d.in_h + d.pad_t + d.pad_b >= d.kh || d.transposed) &&
                 (d.in_w + d.pad_l + d.pad_r >= d.kw || d.transposed) && d.kh * d.kw <= 49;
    if (d.pad_mode == TPG_PAD_REFLECT &&
        (d.pad_t >= d.in_h || d.pad_b >= d.in_h || d.pad_l >= d.in_w || d.pad_r >= d.in_w))
      valid = false;
    // malformed descriptors: one field corrupted
    if (rnd() % 6 == 0) {
      valid = false;
      switch (rnd() % 9) {
        case 0: d.n = -(int)(rnd() % 3); break;
        case 1: d.in_c = 0; break;
        case 2: d.out_c = -1; break;
        case 3: d.kh = 0; break;
        case 4: d.stride_w = 0; break;
        case 5: d.dtype = 3 + rnd() % 5; break;
        case 6: d.out_h += 1 + d.stride_h; break;
        case 7: d.out_w = d.transposed ? d.out_w - 1 : d.out_w + 1; break;
        case 8: d.pad_t = d.pad_l = 200; break;
      }
    }
    // the random walk only asserts on rejection of shapes the planner documents as covered
    run_one(d, valid && d.kh <= 7 && d.kw <= 7 && d.out_h > 0 && d.out_w > 0 && d.in_h > 0);
  }
  (void)tpg_conv2d_workspace(nullptr, TPG_OP_FWD);
  // resize tables: the ends of the size range, the sizes around each output and a seeded sample
  const int outs[5] = {1, 32, 64, 128, 256};
  const int ends[] = {1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 640, 1024, 4095, 4096};
  for (int out : outs) {
    for (int in : ends) resize_table(in, out);
    for (int i = 0; i < 24; ++i) resize_table(1 + (int)(rnd() % 4096), out);
  }
  resize_jobs();
  identity_sweep(iters < 2000 ? iters : 2000);
  landmark_sweep();
  align_sweep();
  printf("planner_asan: %ld valid, %ld rejected descriptors, %ld pack jobs, %ld wgrad plans, %ld data plans, "
         "%ld resize tables, %ld top-k plans, %s\n", g_valid, g_rejected, g_jobs, g_plans, g_dplans, g_tables, g_idplans,
         g_fail ? "FAILED" : "ok");
  return g_fail;
}
