// Inference image path: the generator's [-1, 1] output back to u8 pixels, and the validation
// metrics (PSNR's squared error, SSIM) of a u8 result against the u8 ground truth.
//
//  denorm_u8_kernel       the inverse of crop_norm_kernel's u/255*2-1 (tpg_data.hip), with the
//                         rounding of torchvision.utils.save_image on (x+1)/2: in float32, no FMA
//                         contraction, t = (x + 1) * 127.5 + 0.5; out = NaN ? 0 : clamp(floor(t), 0, 255).
//                         One thread owns four consecutive pixels of the flat [n*h*w] pixel list:
//                         their 4*c output bytes are c whole dwords at a dword-aligned offset
//                         whatever the width is, so every store but the batch's last group is a
//                         dword store.  Loads follow x's contiguous axis: 4-wide along w (NCHW), or
//                         the pixel's channels in 4/2/1-element pieces (channels-last views).
//  metrics_tile_kernel    one block per (image, 16 x 16 pixel tile): the tile plus a 10-pixel apron
//                         to the right and below is staged in LDS for both images; the block sums
//                         (a-b)^2 over its own pixels in integers and, per channel, the SSIM map of
//                         the 11 x 11 windows whose top-left corner lies in the tile, by a row pass
//                         (LDS bytes -> five windowed moments per row) and a column pass.
//  metrics_final_kernel   one block per image adds the tiles' partials in tile order.
//
// SSIM is Wang et al.'s (Gaussian 11 x 11 window of sigma 1.5, valid positions only, C1 = 6.5025,
// C2 = 58.5225, mean over positions and channels).  The five moments sum(w x), sum(w y), sum(w x^2),
// sum(w y^2), sum(w x y) are accumulated in float64: in float32 the raw-moment variance
// sum(w x^2) - mu^2 cancels on flat bright regions (2.7e-4 off on 254 against 254/253 rows), and
// the map, its sum and the mean stay in float64 up to the final float.  Every reduction runs in a
// fixed order (LDS trees, no atomics): reruns are bit-identical.
#include "tpg_internal.h"
#include "../../include/tpgan.h"
#include <math.h>

namespace tpg {
namespace {

// ---------------------------------------------------------------- denorm

struct DenormArgs {
  const void* x;
  int64_t s[4];      // element strides of the logical (n, c, h, w) view
  uint8_t* out;
  int64_t npix;      // n * h * w
  int32_t h, w;
  int32_t roww;      // 1: stride[3] == 1 and rows 4-element aligned where the offset is (NCHW)
  int32_t chv;       // 4 / 2 / 1: stride[1] == 1 and every pixel starts chv-element aligned
  int32_t dword_ok;  // out is 4-byte aligned
};

__device__ __forceinline__ uint32_t quant_u8(float v) {
#pragma clang fp contract(off)
  float t = (v + 1.0f) * 127.5f;
  t = t + 0.5f;
  if (!(t == t)) return 0u;
  t = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);
  return (uint32_t)(int)floorf(t);
}

template <typename E> __device__ __forceinline__ float cvt16(uint16_t b);
template <> __device__ __forceinline__ float cvt16<__bf16>(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }
template <> __device__ __forceinline__ float cvt16<_Float16>(uint16_t b) { return (float)__builtin_bit_cast(_Float16, b); }

// K (1, 2 or 4) consecutive elements at p (K-element aligned) -> float
template <typename E, int K>
__device__ __forceinline__ void load_vec(const E* p, float* f) {
  if constexpr (sizeof(E) == 4) {
    if constexpr (K == 4) {
      const float4 v = *reinterpret_cast<const float4*>(p);
      f[0] = v.x, f[1] = v.y, f[2] = v.z, f[3] = v.w;
    } else if constexpr (K == 2) {
      const float2 v = *reinterpret_cast<const float2*>(p);
      f[0] = v.x, f[1] = v.y;
    } else {
      f[0] = *reinterpret_cast<const float*>(p);
    }
  } else {
    if constexpr (K == 4) {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      f[0] = cvt16<E>((uint16_t)(v.x & 0xffffu)), f[1] = cvt16<E>((uint16_t)(v.x >> 16));
      f[2] = cvt16<E>((uint16_t)(v.y & 0xffffu)), f[3] = cvt16<E>((uint16_t)(v.y >> 16));
    } else if constexpr (K == 2) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
      f[0] = cvt16<E>((uint16_t)(v & 0xffffu)), f[1] = cvt16<E>((uint16_t)(v >> 16));
    } else {
      f[0] = cvt16<E>(*reinterpret_cast<const uint16_t*>(p));
    }
  }
}

// the C channels of the pixel at element offset o
template <typename E, int C>
__device__ __forceinline__ void load_pixel(const E* x, int64_t o, int64_t s1, int chv, float* f) {
  if constexpr (C >= 2) {
    if (chv >= 2) {  // channel stride 1, pixels chv-element aligned
      if constexpr (C == 4) {
        if (chv == 4) {
          load_vec<E, 4>(x + o, f);
          return;
        }
        load_vec<E, 2>(x + o + 2, f + 2);
      }
      if constexpr (C == 3) load_vec<E, 1>(x + o + 2, f + 2);
      load_vec<E, 2>(x + o, f);
      return;
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) load_vec<E, 1>(x + o + c * s1, f + c);
}

template <typename E, int C>
__global__ __launch_bounds__(256) void denorm_u8_kernel(const DenormArgs a) {
  const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= a.npix) return;
  const int np = a.npix - p0 < 4 ? (int)(a.npix - p0) : 4;
  const E* x = reinterpret_cast<const E*>(a.x);
  int xx = (int)(p0 % a.w);
  int64_t q = p0 / a.w;
  int yy = (int)(q % a.h);
  int64_t nn = q / a.h;
  float f[4][C];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int c = 0; c < C; ++c) f[p][c] = 0.f;
  const int64_t o0 = nn * a.s[0] + (int64_t)yy * a.s[2] + (int64_t)xx * a.s[3];
  if (a.roww && np == 4 && xx + 3 < a.w && (o0 & 3) == 0) {
    // four pixels of one row, 4-wide along w per channel
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float v[4];
      load_vec<E, 4>(x + o0 + c * a.s[1], v);
#pragma unroll
      for (int p = 0; p < 4; ++p) f[p][c] = v[p];
    }
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (p < np) {
        load_pixel<E, C>(x, nn * a.s[0] + (int64_t)yy * a.s[2] + (int64_t)xx * a.s[3], a.s[1], a.chv, f[p]);
        if (++xx == a.w) {
          xx = 0;
          if (++yy == a.h) yy = 0, ++nn;
        }
      }
    }
  }
  uint32_t word[C];
#pragma unroll
  for (int k = 0; k < C; ++k) word[k] = 0u;
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int j = p * C + c;  // byte j of the group's 4*C
      word[j >> 2] |= quant_u8(f[p][c]) << (8 * (j & 3));
    }
  uint8_t* o = a.out + p0 * C;
  if (np == 4 && a.dword_ok) {
    uint32_t* ow = reinterpret_cast<uint32_t*>(o);
#pragma unroll
    for (int k = 0; k < C; ++k) ow[k] = word[k];
  } else {
    // the batch's last, partial group (or an output that is not dword aligned): byte stores
#pragma unroll
    for (int j = 0; j < 4 * C; ++j)
      if (j < np * C) o[j] = (uint8_t)(word[j >> 2] >> (8 * (j & 3)));
  }
}

template <typename E>
void launch_denorm(int c, const DenormArgs& a, hipStream_t st) {
  const int64_t groups = (a.npix + 3) / 4;
  const dim3 grid((unsigned)((groups + 255) / 256)), block(256);
  switch (c) {
    case 1: hipLaunchKernelGGL((denorm_u8_kernel<E, 1>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((denorm_u8_kernel<E, 2>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((denorm_u8_kernel<E, 3>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((denorm_u8_kernel<E, 4>), grid, block, 0, st, a); break;
  }
}

// ---------------------------------------------------------------- SSE / SSIM

constexpr int MT = 16;             // tile side (pixels; SSIM windows by their top-left corner)
constexpr int MW = 11;             // SSIM window
constexpr int MA = MT + MW - 1;    // staged side: tile + apron
constexpr int M_THREADS = MT * MT;

struct MetricsArgs {
  const uint8_t* a;
  const uint8_t* b;
  int32_t h, w, c, tiles_x, tiles;
  int32_t ssim;    // 0: squared error only
  double g[MW];    // the normalised 1-D Gaussian
};

struct TilePartial {
  int64_t sse;
  double ssim;     // sum of the map over this tile's windows and all channels
};

__global__ __launch_bounds__(M_THREADS) void metrics_tile_kernel(const MetricsArgs m, TilePartial* part) {
  __shared__ __attribute__((aligned(16))) uint8_t sa[MA * MA * 4];
  __shared__ __attribute__((aligned(16))) uint8_t sb[MA * MA * 4];
  __shared__ double hx[5][MA][MT];  // row-pass moments; reused by the block sums
  const int tid = threadIdx.x;
  const int img = blockIdx.x / m.tiles, tile = blockIdx.x - img * m.tiles;
  const int ty0 = (tile / m.tiles_x) * MT, tx0 = (tile % m.tiles_x) * MT;
  const int C = m.c;
  const int64_t ibase = (int64_t)img * m.h * m.w * C;
  const int rowb = MA * C;  // staged bytes per row
  // does any 11 x 11 window start in this tile?
  const bool win = m.ssim && ty0 + MW <= m.h && tx0 + MW <= m.w;
  const int rows = win ? MA : MT, colb = (win ? MA : MT) * C;
  for (int i = tid; i < rows * colb; i += M_THREADS) {
    const int r = i / colb, k = i - r * colb;  // k = byte inside the staged row segment
    const int y = ty0 + r, xb = tx0 * C + k;
    uint8_t va = 0, vb = 0;
    if (y < m.h && xb < m.w * C) {
      const int64_t o = ibase + ((int64_t)y * m.w) * C + xb;
      va = m.a[o];
      vb = m.b[o];
    }
    sa[r * rowb + k] = va;
    sb[r * rowb + k] = vb;
  }
  __syncthreads();
  const int ly = tid / MT, lx = tid - ly * MT;
  // squared error of this thread's own pixel (staged zeros outside the image add nothing)
  uint32_t se = 0;
  for (int ch = 0; ch < C; ++ch) {
    const int d = (int)sa[ly * rowb + lx * C + ch] - (int)sb[ly * rowb + lx * C + ch];
    se += (uint32_t)(d * d);
  }
  double acc = 0.0;
  if (win) {
    const bool valid = ty0 + ly + MW <= m.h && tx0 + lx + MW <= m.w;
    for (int ch = 0; ch < C; ++ch) {
      // row pass: MA rows x MT window columns
      for (int i = tid; i < MA * MT; i += M_THREADS) {
        const int r = i / MT, cx = i - r * MT;
        double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
        for (int k = 0; k < MW; ++k) {
          const double xa = (double)sa[r * rowb + (cx + k) * C + ch], xb = (double)sb[r * rowb + (cx + k) * C + ch];
          const double wk = m.g[k];
          s0 += wk * xa;
          s1 += wk * xb;
          s2 += wk * (xa * xa);
          s3 += wk * (xb * xb);
          s4 += wk * (xa * xb);
        }
        hx[0][r][cx] = s0, hx[1][r][cx] = s1, hx[2][r][cx] = s2, hx[3][r][cx] = s3, hx[4][r][cx] = s4;
      }
      __syncthreads();
      if (valid) {
        double mu_a = 0, mu_b = 0, aa = 0, bb = 0, ab = 0;
#pragma unroll
        for (int k = 0; k < MW; ++k) {
          const double wk = m.g[k];
          mu_a += wk * hx[0][ly + k][lx];
          mu_b += wk * hx[1][ly + k][lx];
          aa += wk * hx[2][ly + k][lx];
          bb += wk * hx[3][ly + k][lx];
          ab += wk * hx[4][ly + k][lx];
        }
        const double va = aa - mu_a * mu_a, vb = bb - mu_b * mu_b, cov = ab - mu_a * mu_b;
        const double C1 = 6.5025, C2 = 58.5225;
        acc += ((2.0 * mu_a * mu_b + C1) * (2.0 * cov + C2)) / ((mu_a * mu_a + mu_b * mu_b + C1) * (va + vb + C2));
      }
      __syncthreads();
    }
  }
  // block sums in a fixed tree (hx is free again)
  double* rd = &hx[0][0][0];
  uint32_t* ri = reinterpret_cast<uint32_t*>(sa);  // 256 * 4 bytes <= sizeof(sa)
  __syncthreads();
  rd[tid] = acc;
  ri[tid] = se;
  __syncthreads();
  for (int s = M_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      rd[tid] += rd[tid + s];
      ri[tid] += ri[tid + s];  // <= 256 * 4 * 255^2 < 2^32
    }
    __syncthreads();
  }
  if (tid == 0) {
    part[blockIdx.x].sse = (int64_t)ri[0];
    part[blockIdx.x].ssim = rd[0];
  }
}

__global__ __launch_bounds__(64) void metrics_final_kernel(const TilePartial* part, int tiles, double count,
                                                           int64_t* sse, float* ssim) {
  __shared__ int64_t si[64];
  __shared__ double sd[64];
  const TilePartial* p = part + (int64_t)blockIdx.x * tiles;
  int64_t e = 0;
  double s = 0.0;
  for (int t = threadIdx.x; t < tiles; t += 64) {
    e += p[t].sse;
    s += p[t].ssim;
  }
  si[threadIdx.x] = e;
  sd[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 64; ++k) e += si[k], s += sd[k];
    sse[blockIdx.x] = e;
    if (ssim) ssim[blockIdx.x] = (float)(s / count);
  }
}

int metrics_check(const char* fn, int32_t n, int32_t h, int32_t w, int32_t c, int64_t* tiles_x, int64_t* tiles) {
  if (n < 0 || h <= 0 || w <= 0 || h > 32768 || w > 32768)
    return fail(-2, "%s: bad sizes (n >= 0, sides in 1..32768)", fn);
  if (c < 1 || c > 4) return fail(-2, "%s: c must be in 1..4, got %d", fn, c);
  *tiles_x = (w + MT - 1) / MT;
  *tiles = *tiles_x * ((h + MT - 1) / MT);
  if ((int64_t)n * *tiles > 0x7fffffffLL) return fail(-2, "%s: batch too large (n * tiles >= 2^31)", fn);
  return 0;
}

}  // namespace
}  // namespace tpg

using namespace tpg;

extern "C" int32_t tpg_denorm_u8(int32_t n, int32_t c, int32_t h, int32_t w, tpg_tensor x, uint8_t* out,
                                 tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  if (n < 0 || h <= 0 || w <= 0) return fail(-2, "denorm_u8: bad sizes");
  if (c < 1 || c > 4) return fail(-2, "denorm_u8: c must be in 1..4");
  if (x.dtype != TPG_F32 && x.dtype != TPG_BF16 && x.dtype != TPG_F16) return fail(-3, "denorm_u8: bad dtype");
  if (n == 0) return 0;
  if (!x.data || !out) return fail(-10, "denorm_u8: NULL pointer");
  DenormArgs a;
  a.x = x.data;
  for (int i = 0; i < 4; ++i) a.s[i] = x.stride[i];
  a.out = out;
  a.npix = (int64_t)n * h * w;
  a.h = h;
  a.w = w;
  if ((a.npix + 3) / 4 / 256 >= 0x7fffffffLL) return fail(-2, "denorm_u8: batch too large");
  const int es = x.dtype == TPG_F32 ? 4 : 2;
  const uintptr_t addr = (uintptr_t)x.data;
  auto mult = [&](int k) {  // base address and the batch / row / pixel strides k-element aligned
    return addr % ((uintptr_t)es * k) == 0 && x.stride[0] % k == 0 && x.stride[2] % k == 0 && x.stride[3] % k == 0;
  };
  a.chv = 1;
  if (x.stride[1] == 1 && c > 1) a.chv = mult(4) ? 4 : (mult(2) ? 2 : 1);
  // 4-wide along w: the kernel checks each group's own offset, which is 4-aligned for every
  // channel only where the channel stride is too
  a.roww = x.stride[3] == 1 && addr % ((uintptr_t)es * 4) == 0 && (c == 1 || x.stride[1] % 4 == 0);
  a.dword_ok = (uintptr_t)out % 4 == 0;
  hipStream_t st = (hipStream_t)stream;
  if (x.dtype == TPG_F32) launch_denorm<float>(c, a, st);
  else if (x.dtype == TPG_BF16) launch_denorm<__bf16>(c, a, st);
  else launch_denorm<_Float16>(c, a, st);
  return launched("denorm_u8");
}

extern "C" int64_t tpg_image_metrics_workspace(int32_t n, int32_t h, int32_t w, int32_t c) {
  int64_t tx, tiles;
  const int rc = metrics_check("image_metrics_workspace", n, h, w, c, &tx, &tiles);
  if (rc) return rc;
  return (int64_t)sizeof(TilePartial) * (n > 0 ? n : 1) * tiles;
}

extern "C" int32_t tpg_image_metrics_u8(int32_t n, int32_t h, int32_t w, int32_t c, const uint8_t* a,
                                        const uint8_t* b, int64_t* sse, float* ssim, void* ws, size_t ws_bytes,
                                        tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  int64_t tx, tiles;
  const int rc = metrics_check("image_metrics_u8", n, h, w, c, &tx, &tiles);
  if (rc) return rc;
  if (ssim && (h < MW || w < MW)) return fail(-2, "image_metrics_u8: SSIM needs h and w >= 11");
  if (n == 0) return 0;
  if (!a || !b || !sse || !ws) return fail(-10, "image_metrics_u8: NULL pointer");
  if ((uintptr_t)ws % 8 != 0) return fail(-4, "image_metrics_u8: workspace must be 8-byte aligned");
  if (ws_bytes < sizeof(TilePartial) * (size_t)n * (size_t)tiles)
    return fail(-4, "image_metrics_u8: workspace too small (tpg_image_metrics_workspace)");
  MetricsArgs m;
  m.a = a;
  m.b = b;
  m.h = h;
  m.w = w;
  m.c = c;
  m.tiles_x = (int32_t)tx;
  m.tiles = (int32_t)tiles;
  m.ssim = ssim ? 1 : 0;
  double sum = 0.0;
  for (int k = 0; k < MW; ++k) {
    m.g[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
    sum += m.g[k];
  }
  for (int k = 0; k < MW; ++k) m.g[k] /= sum;
  hipStream_t st = (hipStream_t)stream;
  TilePartial* part = reinterpret_cast<TilePartial*>(ws);
  hipLaunchKernelGGL(metrics_tile_kernel, dim3((unsigned)(n * tiles)), dim3(M_THREADS), 0, st, m, part);
  if (int32_t e = launched("image_metrics_u8")) return e;
  const double count = ssim ? (double)c * (h - MW + 1) * (double)(w - MW + 1) : 1.0;
  hipLaunchKernelGGL(metrics_final_kernel, dim3((unsigned)n), dim3(64), 0, st, (const TilePartial*)part, (int)tiles,
                     count, sse, ssim);
  return launched("image_metrics_u8");
}
