// Face alignment between the landmark detector and the generator: fit a similarity transform
// from the detected points to a canonical template, and resample the photo through it.
//
//   similarity_fit_kernel  least-squares rotation + uniform scale + translation (no reflection)
//                          that maps the template points q (output frame, the same for every face)
//                          onto a face's points p (photo pixels): the direction the warp samples
//                          in, so nothing is inverted.  Closed form in float32, one face per lane:
//                            qc = q - mean(q), pc = p - mean(p), S = sum |qc|^2
//                            a = sum(qc.x*pc.x + qc.y*pc.y) / S,  b = sum(qc.x*pc.y - qc.y*pc.x) / S
//                            M = [[a, -b], [b, a]],  t = mean(p) - M * mean(q)
//                          mean(q), qc and S are the host's (float32, index order); sums over the K
//                          points run in index order, divisions are IEEE, no FMA contraction.
//   affine_warp_kernel     out[b] = the photo of job b sampled through its 16.16 matrix, n x n
//                          bilinear sub-samples per output pixel (n from the matrix: no aliasing when
//                          the map shrinks the photo), edge replicate.  Integer arithmetic only, as
//                          the LANCZOS resize: bit-exact against an integer restatement.
//
// The warp's sample positions (tpgan.h states them as one floor division per sub-sample):
//   X = tx + floor((m00*U + m01*V) / 2n) - 32768,  U = 2n*ox + 2i + 1,  V = 2n*oy + 2j + 1
// With m = A*2n + R (floor division, 0 <= R < 2n) the numerator is
//   2n * (m00*ox + m01*oy + A00*(2i+1) + A01*(2j+1)) + R00*(2i+1) + R01*(2j+1)
// so the floor is the bracket plus (R00*(2i+1) + R01*(2j+1)) / 2n, a quotient of two small
// non-negative ints: the 64-bit division leaves the pixel loop and the result is the same integer.
//
// Memory: a block is one 16 x 16 output tile of one face, so its source footprint is a small
// parallelogram that stays in the vector L1; taps are byte loads at clamped coordinates, never
// outside [src, src + (H-1)*row_stride + W*3).  One thread writes the 3 bytes of its pixel.
#include <cmath>
#include <cstring>

#include "tpg_internal.h"
#include "../../include/tpgan.h"

namespace tpg {
namespace {

constexpr int AL_MAX = 4096;   // largest side, photo or output
constexpr int AL_KMAX = 8;     // most template points
constexpr int AL_TILE = 16;    // output tile side: 256 threads, one pixel each
constexpr int AL_NMAX = 16;    // most sub-samples per axis

struct FitArgs {
  float qcx[AL_KMAX], qcy[AL_KMAX];  // centred template
  float qmx, qmy, S;
};

struct WarpJob {                 // tpg_warp_job_bytes() == 32; layout documented in tpgan.h
  const uint8_t* src;
  int64_t row_stride;            // bytes
  int32_t h, w, out_h, out_w;
};
static_assert(sizeof(WarpJob) == 32, "job record layout");

__global__ void similarity_fit_kernel(int B, int K, FitArgs q, const float* __restrict__ pts,
                                      const int32_t* __restrict__ in_status, float* __restrict__ mat,
                                      int32_t* __restrict__ mat_q16, int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= B) return;
  const float* p = pts + (int64_t)f * K * 2;
  float px[AL_KMAX], py[AL_KMAX];
  int st = 0;
  float sx = 0.f, sy = 0.f;
  for (int k = 0; k < AL_KMAX; ++k) {
    if (k < K) {
      px[k] = p[2 * k];
      py[k] = p[2 * k + 1];
      if (!(fabsf(px[k]) <= 1.0e9f) || !(fabsf(py[k]) <= 1.0e9f)) st |= 1;  // NaN fails the comparison
      sx = sx + px[k];
      sy = sy + py[k];
    }
  }
  const float pmx = sx / (float)K, pmy = sy / (float)K;
  float sa = 0.f, sb = 0.f;
  for (int k = 0; k < AL_KMAX; ++k) {
    if (k < K) {
      const float cx = px[k] - pmx, cy = py[k] - pmy;
      sa = sa + (q.qcx[k] * cx + q.qcy[k] * cy);
      sb = sb + (q.qcx[k] * cy - q.qcy[k] * cx);
    }
  }
  float a = sa / q.S, b = sb / q.S;
  float tx = pmx - (a * q.qmx - b * q.qmy);
  float ty = pmy - (b * q.qmx + a * q.qmy);
  if (!st) {
    const float n2 = a * a + b * b;
    // NaN fails every comparison: each test is written so that NaN sets the bit
    if (!(n2 > 0.f) || !(n2 <= 3.0e38f) || !(sqrtf(n2) <= 32.f) || !(fabsf(tx) < 16384.f) || !(fabsf(ty) < 16384.f))
      st |= 2;
  }
  if (st) {
    a = 1.f;
    b = 0.f;
    tx = 0.f;
    ty = 0.f;
  }
  if (in_status && in_status[f] != 0) st |= 4;
  const float m[6] = {a, -b, tx, b, a, ty};
  for (int k = 0; k < 6; ++k) {
    mat[(int64_t)f * 6 + k] = m[k];
    mat_q16[(int64_t)f * 6 + k] = __float2int_rn(m[k] * 65536.0f);
  }
  status[f] = st;
}

__device__ __forceinline__ int al_floor_div(int v, int d) {  // d > 0
  const int q = v / d;
  return (v % d != 0 && v < 0) ? q - 1 : q;
}

__device__ __forceinline__ int al_clamp(int64_t v, int hi) {
  return v < 0 ? 0 : (v > hi ? hi : (int)v);
}

__global__ __launch_bounds__(AL_TILE* AL_TILE) void affine_warp_kernel(const WarpJob* __restrict__ jobs,
                                                                       const int32_t* __restrict__ mats, int out_h,
                                                                       int out_w, uint8_t* __restrict__ out,
                                                                       int32_t* __restrict__ status) {
  const int b = blockIdx.z;
  const WarpJob j = jobs[b];
  if (j.out_h != out_h || j.out_w != out_w) return;
  if (j.w < 1 || j.w > AL_MAX || j.h < 1 || j.h > AL_MAX) return;  // not a tpg_warp_pack_job record
  const int32_t* m = mats + (int64_t)b * 6;
  const int m00 = m[0], m01 = m[1], m10 = m[3], m11 = m[4];
  const int64_t tx = m[2], ty = m[5];
  // squares of int32 reach 2^62 and their sum 2^63: unsigned
  const uint64_t c0 = (uint64_t)((int64_t)m00 * m00) + (uint64_t)((int64_t)m10 * m10);
  const uint64_t c1 = (uint64_t)((int64_t)m01 * m01) + (uint64_t)((int64_t)m11 * m11);
  const uint64_t d = c0 > c1 ? c0 : c1;
  int n = 0;
  for (int k = 1; k <= AL_NMAX && !n; ++k) {
    const uint64_t s = (uint64_t)k << 16;
    if (s * s >= d) n = k;
  }
  const bool under = n == 0;
  if (under) n = AL_NMAX;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) status[b] = under ? 8 : 0;
  const int ox = blockIdx.x * AL_TILE + (threadIdx.x & (AL_TILE - 1));
  const int oy = blockIdx.y * AL_TILE + (threadIdx.x / AL_TILE);
  if (ox >= out_w || oy >= out_h) return;
  const int n2 = 2 * n;
  const int a00 = al_floor_div(m00, n2), a01 = al_floor_div(m01, n2);
  const int a10 = al_floor_div(m10, n2), a11 = al_floor_div(m11, n2);
  const int r00 = m00 - a00 * n2, r01 = m01 - a01 * n2, r10 = m10 - a10 * n2, r11 = m11 - a11 * n2;  // 0..2n-1
  const int64_t bx = tx - 32768 + (int64_t)m00 * ox + (int64_t)m01 * oy;
  const int64_t by = ty - 32768 + (int64_t)m10 * ox + (int64_t)m11 * oy;
  const int wmax = j.w - 1, hmax = j.h - 1;
  uint32_t acc0 = 0, acc1 = 0, acc2 = 0;  // at most 255 * 65536 * 256 < 2^32
  for (int sj = 0; sj < n; ++sj) {
    const int v = 2 * sj + 1;
    for (int si = 0; si < n; ++si) {
      const int u = 2 * si + 1;
      const int64_t X = bx + (int64_t)a00 * u + (int64_t)a01 * v + (int)((uint32_t)(r00 * u + r01 * v) / (uint32_t)n2);
      const int64_t Y = by + (int64_t)a10 * u + (int64_t)a11 * v + (int)((uint32_t)(r10 * u + r11 * v) / (uint32_t)n2);
      const uint32_t fx = (uint32_t)(X >> 8) & 255u, fy = (uint32_t)(Y >> 8) & 255u;
      const int64_t ix = X >> 16, iy = Y >> 16;
      const int x0 = al_clamp(ix, wmax) * 3, x1 = al_clamp(ix + 1, wmax) * 3;
      const uint8_t* row0 = j.src + (int64_t)al_clamp(iy, hmax) * j.row_stride;
      const uint8_t* row1 = j.src + (int64_t)al_clamp(iy + 1, hmax) * j.row_stride;
      const uint32_t w00 = (256u - fx) * (256u - fy), w01 = fx * (256u - fy);
      const uint32_t w10 = (256u - fx) * fy, w11 = fx * fy;
      acc0 += w00 * row0[x0] + w01 * row0[x1] + w10 * row1[x0] + w11 * row1[x1];
      acc1 += w00 * row0[x0 + 1] + w01 * row0[x1 + 1] + w10 * row1[x0 + 1] + w11 * row1[x1 + 1];
      acc2 += w00 * row0[x0 + 2] + w01 * row0[x1 + 2] + w10 * row1[x0 + 2] + w11 * row1[x1 + 2];
    }
  }
  // (acc + 32768*n*n) / (65536*n*n): the shift first, then a 32-bit division (nested floors agree)
  const uint32_t nn = (uint32_t)(n * n);
  const uint64_t half = (uint64_t)32768 * nn;
  uint8_t* o = out + (((int64_t)b * out_h + oy) * out_w + ox) * 3;
  o[0] = (uint8_t)((uint32_t)(((uint64_t)acc0 + half) >> 16) / nn);
  o[1] = (uint8_t)((uint32_t)(((uint64_t)acc1 + half) >> 16) / nn);
  o[2] = (uint8_t)((uint32_t)(((uint64_t)acc2 + half) >> 16) / nn);
}

bool al_size_ok(int v) { return v >= 1 && v <= AL_MAX; }

}  // namespace

int launch_similarity_fit(int B, int K, const float* tmpl, const float* points, const int* in_status, float* matrix,
                          int* matrix_q16, int* status, hipStream_t s) {
#pragma clang fp contract(off)
  FitArgs q;
  memset(&q, 0, sizeof(q));
  float sx = 0.f, sy = 0.f;
  for (int k = 0; k < K; ++k) {
    sx = sx + tmpl[2 * k];
    sy = sy + tmpl[2 * k + 1];
  }
  q.qmx = sx / (float)K;
  q.qmy = sy / (float)K;
  float S = 0.f;
  for (int k = 0; k < K; ++k) {
    q.qcx[k] = tmpl[2 * k] - q.qmx;
    q.qcy[k] = tmpl[2 * k + 1] - q.qmy;
    S = S + (q.qcx[k] * q.qcx[k] + q.qcy[k] * q.qcy[k]);
  }
  q.S = S;
  if (!(S > 0.f) || !std::isfinite(S)) return -1;
  hipLaunchKernelGGL(similarity_fit_kernel, dim3((B + 63) / 64), dim3(64), 0, s, B, K, q, points, in_status, matrix,
                     matrix_q16, status);
  return (int)hipGetLastError();
}

int launch_affine_warp_u8(int njobs, const void* jobs_dev, const int* matrix_q16, int out_h, int out_w, uint8_t* out,
                          int* status, hipStream_t s) {
  const dim3 grid((out_w + AL_TILE - 1) / AL_TILE, (out_h + AL_TILE - 1) / AL_TILE, njobs);
  hipLaunchKernelGGL(affine_warp_kernel, grid, dim3(AL_TILE * AL_TILE), 0, s, static_cast<const WarpJob*>(jobs_dev),
                     matrix_q16, out_h, out_w, out, status);
  return (int)hipGetLastError();
}

}  // namespace tpg

using namespace tpg;

extern "C" int32_t tpg_similarity_fit(int32_t B, int32_t K, const float* points, const float* tmpl,
                                      const int32_t* in_status, float* matrix, int32_t* matrix_q16, int32_t* status,
                                      tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  if (B == 0) return 0;
  if (B < 0) return fail(-2, "similarity_fit: negative face count");
  if (K < 2 || K > AL_KMAX) return fail(-2, "similarity_fit: K must be in 2..8, got %d", K);
  if (!points || !tmpl || !matrix || !matrix_q16 || !status) return fail(-10, "similarity_fit: NULL pointer");
  for (int k = 0; k < 2 * K; ++k)
    if (!std::isfinite(tmpl[k])) return fail(-2, "similarity_fit: template coordinate %d is not finite", k);
  const int e = launch_similarity_fit(B, K, tmpl, points, in_status, matrix, matrix_q16, status, (hipStream_t)stream);
  if (e == -1) return fail(-2, "similarity_fit: the template points coincide (or their spread overflows float32)");
  return hip_check(e, "similarity_fit");
}

extern "C" size_t tpg_warp_job_bytes(void) { return sizeof(WarpJob); }

extern "C" int32_t tpg_warp_pack_job(void* jobs, int32_t index, const uint8_t* src, int32_t h, int32_t w, int32_t bands,
                                     int64_t row_stride, int32_t out_h, int32_t out_w) {
  if (!jobs || !src) return fail(-10, "warp_pack_job: NULL pointer");
  if (index < 0) return fail(-2, "warp_pack_job: negative job index");
  if (bands != 3) return fail(-2, "warp_pack_job: images must have 3 interleaved bands (RGB)");
  if (!al_size_ok(h) || !al_size_ok(w) || !al_size_ok(out_h) || !al_size_ok(out_w))
    return fail(-2, "warp_pack_job: sizes must be in 1..4096");
  if (row_stride < (int64_t)w * 3) return fail(-2, "warp_pack_job: row stride smaller than W*3 bytes");
  WarpJob j;
  j.src = src;
  j.row_stride = row_stride;
  j.h = h;
  j.w = w;
  j.out_h = out_h;
  j.out_w = out_w;
  memcpy(static_cast<char*>(jobs) + (size_t)index * sizeof(WarpJob), &j, sizeof(j));
  return 0;
}

extern "C" int32_t tpg_affine_warp_u8(int32_t njobs, const void* jobs_dev, const int32_t* matrix_q16, int32_t out_h,
                                      int32_t out_w, uint8_t* out, int32_t* status, tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  if (njobs == 0) return 0;
  if (njobs < 0 || njobs > 65535) return fail(-2, "affine_warp_u8: 0..65535 jobs per call, got %d", njobs);
  if (!al_size_ok(out_h) || !al_size_ok(out_w)) return fail(-2, "affine_warp_u8: sizes must be in 1..4096");
  if (!jobs_dev || !matrix_q16 || !out || !status) return fail(-10, "affine_warp_u8: NULL pointer");
  return hip_check(launch_affine_warp_u8(njobs, jobs_dev, matrix_q16, out_h, out_w, out, status, (hipStream_t)stream),
                   "affine_warp_u8");
}
