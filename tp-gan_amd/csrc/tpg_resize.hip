// Pillow's 8-bit LANCZOS resize (Image.resize(size, Image.LANCZOS) on an RGB image), bit for
// bit, for a batch of images of different sizes: TestDataset's 128 / 64 / 32 images
// (DataAndDataset.py:247-251), the last per-sample pixel work the data path did on the host.
//
// Pillow's resampler is integer arithmetic over coefficient tables computed in double:
//   host    tpg_resize_coeffs   per axis and (in, out) pair: bounds (xmin, n) and the normalised
//                               window weights rounded to 22 fractional bits
//   device  resize_h_kernel     along W: every source row -> a u8 row of out_w pixels
//           resize_v_kernel     along H, on the ROUNDED u8 image the first pass left
//   out = clamp(((1 << 21) + sum_x src[xmin + x] * k[x]) >> 22, 0, 255), sums in int32
// A pass whose in == out is skipped (not run with identity weights): the horizontal kernel
// leaves such a job alone and the vertical kernel reads the source directly; a job with
// H == out_h gets its horizontal rows written straight into the output, and a job with both
// sizes equal is copied by the vertical launch.  Two launches per call whatever the batch holds.
//
// There is no floating point on the device.  Pixels are 8 bits and the coefficients are checked
// on the host to fit 24 signed bits, so every product is a v_mad_i32_i24.
//
// Memory: source rows are W*3 bytes and start at any byte address.  The horizontal kernel
// stages rows in LDS with dword loads over the 4-byte aligned body of each row, picked from
// the row's real address, and byte loads for the up to 3 + 3 bytes around it; it never touches
// a byte outside [row, row + W*3).  The vertical kernel reads 4 neighbouring bytes of a row as
// one dword only where that address is aligned and all 4 lie inside the row.
#include <cmath>
#include <cstring>
#include <vector>

#include "tpg_internal.h"
#include "../../include/tpgan.h"

namespace tpg {
namespace {

constexpr int RS_MAX = 4096;       // largest side, in or out
constexpr int RS_PB = 22;          // fractional bits of a coefficient (Pillow's PRECISION_BITS)
constexpr int RS_THREADS = 256;
constexpr int RS_LDS = 32768;      // bytes of staged source rows per block
constexpr int RS_ROWS = 8;         // at most this many rows per block iteration

struct ResizeJob {                 // tpg_resize_job_bytes() == 64; layout documented in tpgan.h
  const uint8_t* src;
  int64_t row_stride;              // bytes
  int64_t tab_h, tab_v;            // int32 offsets of the axis tables in the table buffer
  int64_t ws_off;                  // byte offset of the intermediate image in the workspace
  int32_t h, w, out_h, out_w;
  int32_t ksize_h, ksize_v;
};
static_assert(sizeof(ResizeJob) == 64, "job record layout");

// pixel (8 bits) * coefficient (24 signed bits) + sum: one v_mad_i32_i24
__device__ __forceinline__ int rs_mad(int px, int k, int acc) { return __mul24(px, k) + acc; }

// clamp(ss >> 22, 0, 255): the sum is clamped first, so a negative one ends at 0 as Pillow's
// arithmetic shift leaves it, and the shift is a plain logical one.  (Shift-then-clamp pairs
// ORed into a word compile to v_ashr_pk_u8_i32, whose upper half hipcc takes to be zero; on
// MI355X bytes 2 and 3 of such words came out wrong.  This form does not select it.)
__device__ __forceinline__ uint32_t rs_clip(int ss) {
  const int hi = (256 << RS_PB) - 1;
  ss = ss < 0 ? 0 : (ss > hi ? hi : ss);
  return (uint32_t)ss >> RS_PB;
}

__global__ __launch_bounds__(RS_THREADS) void resize_h_kernel(const ResizeJob* __restrict__ jobs,
                                                              const int32_t* __restrict__ tables, int out_h,
                                                              int out_w, uint8_t* __restrict__ out,
                                                              uint8_t* __restrict__ ws) {
  __shared__ uint32_t lds[RS_LDS / 4];
  const ResizeJob j = jobs[blockIdx.x];
  if (j.out_h != out_h || j.out_w != out_w || j.w == out_w) return;
  if (j.w < 1 || j.w > RS_MAX || j.h < 1 || j.h > RS_MAX) return;  // not a tpg_resize_pack_job record
  const int tid = threadIdx.x;
  const int rowb = j.w * 3;
  const int pitch = (rowb + 6) & ~3;  // a row keeps its address phase (0..3) in LDS
  const int rb = RS_LDS / pitch < RS_ROWS ? RS_LDS / pitch : RS_ROWS;  // >= 2 at W = 4096
  uint8_t* dst = j.h == out_h ? out + (int64_t)blockIdx.x * out_h * out_w * 3 : ws + j.ws_off;
  const int32_t* bounds = tables + j.tab_h;
  const int32_t* coef = bounds + 2 * out_w;
  uint8_t* l8 = reinterpret_cast<uint8_t*>(lds);
  const int nchunk = (j.h + rb - 1) / rb;
  for (int ch = blockIdx.y; ch < nchunk; ch += gridDim.y) {
    const int y0 = ch * rb;
    const int nr = j.h - y0 < rb ? j.h - y0 : rb;
    __syncthreads();  // the previous chunk's rows are no longer read
    for (int r = 0; r < nr; ++r) {
      const uint8_t* g = j.src + (int64_t)(y0 + r) * j.row_stride;
      const int head = (int)((uintptr_t)g & 3);
      int nh = (4 - head) & 3;  // bytes before the first aligned dword
      if (nh > rowb) nh = rowb;
      const int nd = (rowb - nh) >> 2;           // whole aligned dwords inside the row
      const int nt = rowb - nh - 4 * nd;         // bytes after the last one
      uint8_t* l = l8 + r * pitch + head;        // l[i] = byte i of the row; l + nh is 4-aligned
      const uint32_t* g4 = reinterpret_cast<const uint32_t*>(g + nh);
      uint32_t* l4 = reinterpret_cast<uint32_t*>(l + nh);
      for (int i = tid; i < nd; i += RS_THREADS) l4[i] = g4[i];
      if (tid < nh) l[tid] = g[tid];
      if (tid >= 64 && tid - 64 < nt) l[nh + 4 * nd + tid - 64] = g[nh + 4 * nd + tid - 64];
    }
    __syncthreads();
    for (int it = tid; it < nr * out_w; it += RS_THREADS) {
      const int r = it / out_w, xx = it - r * out_w;
      const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
      const int32_t* k = coef + (int64_t)xx * j.ksize_h;
      const int head = (int)((uintptr_t)(j.src + (int64_t)(y0 + r) * j.row_stride) & 3);
      const uint8_t* p = l8 + r * pitch + head + xmin * 3;
      int a0 = 1 << (RS_PB - 1), a1 = a0, a2 = a0;
      for (int x = 0; x < n; ++x) {
        const int kk = k[x];
        a0 = rs_mad((int)p[3 * x], kk, a0);
        a1 = rs_mad((int)p[3 * x + 1], kk, a1);
        a2 = rs_mad((int)p[3 * x + 2], kk, a2);
      }
      uint8_t* o = dst + ((int64_t)(y0 + r) * out_w + xx) * 3;
      o[0] = (uint8_t)rs_clip(a0);
      o[1] = (uint8_t)rs_clip(a1);
      o[2] = (uint8_t)rs_clip(a2);
    }
  }
}

__global__ __launch_bounds__(RS_THREADS) void resize_v_kernel(const ResizeJob* __restrict__ jobs,
                                                              const int32_t* __restrict__ tables, int out_h,
                                                              int out_w, uint8_t* __restrict__ out,
                                                              const uint8_t* __restrict__ ws) {
  const ResizeJob j = jobs[blockIdx.x];
  if (j.out_h != out_h || j.out_w != out_w) return;
  if (j.w < 1 || j.w > RS_MAX || j.h < 1 || j.h > RS_MAX) return;
  const bool copy = j.h == out_h;
  if (copy && j.w != out_w) return;  // the horizontal pass wrote the output
  const int ncols = out_w * 3;
  const uint8_t* s = j.w == out_w ? j.src : ws + j.ws_off;
  const int64_t S = j.w == out_w ? j.row_stride : ncols;
  uint8_t* o = out + (int64_t)blockIdx.x * out_h * ncols;
  const int32_t* bounds = tables + j.tab_v;
  const int32_t* coef = bounds + 2 * out_h;
  const int ng = (ncols + 3) >> 2;  // groups of 4 neighbouring bytes of a row
  const int items = out_h * ng;
  for (int it = blockIdx.y * RS_THREADS + threadIdx.x; it < items; it += gridDim.y * RS_THREADS) {
    const int yy = it / ng, c0 = (it - yy * ng) * 4;
    const int nc = ncols - c0 < 4 ? ncols - c0 : 4;
    // both passes skipped: one tap of weight 1.0 gives the source byte back
    const int ymin = copy ? yy : bounds[2 * yy], n = copy ? 1 : bounds[2 * yy + 1];
    const int32_t* k = coef + (int64_t)yy * j.ksize_v;
    const uint8_t* p = s + (int64_t)ymin * S + c0;
    const bool wide = nc == 4 && (((uintptr_t)p | (uintptr_t)S) & 3) == 0;
    int a[4];
    for (int c = 0; c < 4; ++c) a[c] = 1 << (RS_PB - 1);
    if (wide) {
      for (int y = 0; y < n; ++y) {
        const int kk = copy ? 1 << RS_PB : k[y];
        const uint32_t u = *reinterpret_cast<const uint32_t*>(p + y * S);
        a[0] = rs_mad((int)(u & 255u), kk, a[0]);
        a[1] = rs_mad((int)((u >> 8) & 255u), kk, a[1]);
        a[2] = rs_mad((int)((u >> 16) & 255u), kk, a[2]);
        a[3] = rs_mad((int)(u >> 24), kk, a[3]);
      }
    } else {
      for (int y = 0; y < n; ++y) {
        const int kk = copy ? 1 << RS_PB : k[y];
        for (int c = 0; c < nc; ++c) a[c] = rs_mad((int)p[y * S + c], kk, a[c]);
      }
    }
    uint8_t* q = o + (int64_t)yy * ncols + c0;
    if (nc == 4 && ((uintptr_t)q & 3) == 0) {
      *reinterpret_cast<uint32_t*>(q) = rs_clip(a[0]) | rs_clip(a[1]) << 8 |
                                        rs_clip(a[2]) << 16 | rs_clip(a[3]) << 24;
    } else {
      for (int c = 0; c < nc; ++c) q[c] = (uint8_t)rs_clip(a[c]);
    }
  }
}

bool size_ok(int v) { return v >= 1 && v <= RS_MAX; }

double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}

double lanczos_filter(double x) {
  if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3.0);
  return 0.0;
}

int ksize_of(int in_size, int out_size) {
  const double scale = (double)in_size / (double)out_size;
  const double support = 3.0 * (scale < 1.0 ? 1.0 : scale);
  return (int)ceil(support) * 2 + 1;
}

}  // namespace
}  // namespace tpg

using namespace tpg;

extern "C" int32_t tpg_resize_ksize(int32_t in_size, int32_t out_size) {
  if (!size_ok(in_size) || !size_ok(out_size)) {
    fail(-2, "resize_ksize: sizes must be in 1..4096");
    return 0;
  }
  return ksize_of(in_size, out_size);
}

extern "C" int64_t tpg_resize_table_ints(int32_t in_size, int32_t out_size) {
  if (!size_ok(in_size) || !size_ok(out_size)) {
    fail(-2, "resize_table_ints: sizes must be in 1..4096");
    return 0;
  }
  return (int64_t)out_size * (2 + ksize_of(in_size, out_size));
}

extern "C" int32_t tpg_resize_coeffs(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* coeffs) {
#pragma clang fp contract(off)
  if (!size_ok(in_size) || !size_ok(out_size)) return fail(-2, "resize_coeffs: sizes must be in 1..4096");
  if (!bounds || !coeffs) return fail(-10, "resize_coeffs: NULL pointer");
  const double scale = (double)in_size / (double)out_size;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 3.0 * fs;
  const int ksize = (int)ceil(support) * 2 + 1;
  const double ss = 1.0 / fs;  // Pillow multiplies by the reciprocal; x / fs can differ in the last bit
  std::vector<double> w(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    const int n = xmax - xmin;
    if (n < 0 || n > ksize) return fail(-2, "resize_coeffs: window outside the table");
    double tot = 0.0;
    for (int x = 0; x < n; ++x) {
      w[x] = lanczos_filter((x + xmin - center + 0.5) * ss);
      tot += w[x];
    }
    int32_t* k = coeffs + (int64_t)xx * ksize;
    for (int x = 0; x < n; ++x) {
      const double v = tot != 0.0 ? w[x] / tot : w[x];
      const double f = v < 0 ? v * (double)(1 << RS_PB) - 0.5 : v * (double)(1 << RS_PB) + 0.5;
      // the kernels multiply with the 24-bit multiply-add
      if (!(f > -8388608.0 && f < 8388608.0)) return fail(-2, "resize_coeffs: coefficient exceeds 24 bits");
      k[x] = (int32_t)f;
    }
    for (int x = n; x < ksize; ++x) k[x] = 0;
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = n;
  }
  return 0;
}

extern "C" size_t tpg_resize_job_bytes(void) { return sizeof(ResizeJob); }

extern "C" int64_t tpg_resize_workspace(int32_t h, int32_t w, int32_t out_h, int32_t out_w) {
  if (!size_ok(h) || !size_ok(w) || !size_ok(out_h) || !size_ok(out_w))
    return fail(-2, "resize_workspace: sizes must be in 1..4096");
  if (w == out_w || h == out_h) return 0;  // one pass at most: no intermediate image
  return ((int64_t)h * out_w * 3 + 15) & ~(int64_t)15;
}

extern "C" int32_t tpg_resize_pack_job(void* jobs, int32_t index, const uint8_t* src, int32_t h, int32_t w,
                                       int32_t bands, int64_t row_stride, int32_t out_h, int32_t out_w,
                                       int64_t tab_h, int64_t tab_v, int64_t ws_off) {
  if (!jobs || !src) return fail(-10, "resize_pack_job: NULL pointer");
  if (index < 0) return fail(-2, "resize_pack_job: negative job index");
  if (bands != 3) return fail(-2, "resize_pack_job: images must have 3 interleaved bands (RGB)");
  if (!size_ok(h) || !size_ok(w) || !size_ok(out_h) || !size_ok(out_w))
    return fail(-2, "resize_pack_job: sizes must be in 1..4096");
  if (row_stride < (int64_t)w * 3) return fail(-2, "resize_pack_job: row stride smaller than W*3 bytes");
  if ((w != out_w && tab_h < 0) || (h != out_h && tab_v < 0))
    return fail(-2, "resize_pack_job: negative table offset");
  if (w != out_w && h != out_h && (ws_off < 0 || (ws_off & 15)))
    return fail(-2, "resize_pack_job: workspace offset must be a non-negative multiple of 16");
  ResizeJob j;
  j.src = src;
  j.row_stride = row_stride;
  j.tab_h = w != out_w ? tab_h : 0;
  j.tab_v = h != out_h ? tab_v : 0;
  j.ws_off = w != out_w && h != out_h ? ws_off : 0;
  j.h = h;
  j.w = w;
  j.out_h = out_h;
  j.out_w = out_w;
  j.ksize_h = ksize_of(w, out_w);
  j.ksize_v = ksize_of(h, out_h);
  memcpy(static_cast<char*>(jobs) + (size_t)index * sizeof(ResizeJob), &j, sizeof(j));
  return 0;
}

extern "C" int32_t tpg_resize_u8(int32_t njobs, const void* jobs_dev, const int32_t* tables_dev, int32_t out_h,
                                 int32_t out_w, uint8_t* out, void* ws, tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  if (njobs == 0) return 0;
  if (njobs < 0 || !size_ok(out_h) || !size_ok(out_w)) return fail(-2, "resize_u8: bad sizes");
  if (!jobs_dev || !tables_dev || !out) return fail(-10, "resize_u8: NULL pointer");
  // blocks of a job stride over its row chunks / output groups, so the grid needs no image size
  int per_job = 4096 / njobs;
  per_job = per_job < 1 ? 1 : (per_job > 512 ? 512 : per_job);
  const dim3 grid(njobs, per_job);
  const ResizeJob* jobs = static_cast<const ResizeJob*>(jobs_dev);
  hipLaunchKernelGGL(resize_h_kernel, grid, dim3(RS_THREADS), 0, (hipStream_t)stream, jobs, tables_dev, out_h, out_w,
                     out, static_cast<uint8_t*>(ws));
  hipLaunchKernelGGL(resize_v_kernel, grid, dim3(RS_THREADS), 0, (hipStream_t)stream, jobs, tables_dev, out_h, out_w,
                     out, static_cast<const uint8_t*>(ws));
  return launched("resize_u8");
}
