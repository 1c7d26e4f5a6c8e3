// Identity scoring: unit-length embeddings, a fused cosine-similarity + top-k search that never
// stores the P x G similarity matrix, and a pairwise cosine.
//
//  l2_normalize_kernel    one wave per row of a strided f32 / bf16 / f16 [n][d] view: sum of squares
//                         in f32 (each lane its elements d = lane, lane + 64, ... in order, then a
//                         xor butterfly over the 64 lanes), out = x / sqrt(ss) as contiguous f32
//                         [n][dpad] with zero pad columns.
//  cosine_topk_kernel     a block owns 128 probes x one chunk of the gallery.  It walks the chunk
//                         in tiles of 128 gallery rows and each tile along d in steps of 32: both
//                         operands go global -> registers (the next step's loads are in flight
//                         under this step's MFMAs) -> LDS rows of 36 floats (16-byte reads of 32
//                         consecutive rows fall on distinct banks).  Wave w owns probes 32w..32w+31
//                         against all 128 gallery rows: four 32 x 32 accumulators of
//                         v_mfma_f32_32x32x2_f32 with the GALLERY as the A operand, so that a lane
//                         ends up with one probe (its column) and 64 gallery rows (its registers).
//                         Each lane therefore keeps its probe's running top-8 in registers across
//                         the whole chunk -- a compare against the 8th score per candidate, an
//                         unrolled insertion when it passes -- and nothing crosses lanes until the
//                         chunk ends: lanes l and l + 32 (the two halves of a probe's rows) merge by
//                         one exchange and the probe's first k entries go to the workspace.
//  cosine_merge_kernel    one thread per probe merges its partial lists in chunk order.
//  cosine_pairs_kernel    one wave per pair of rows: dot, |a|^2 and |b|^2 in f32, same reduction.
//
// The f32-input MFMA is a k-ordered fmaf chain (one rounding per product): the score of a (probe,
// gallery row) pair depends on neither the tile position nor the chunk length, so duplicate
// gallery rows score bit-equal and every gchunk gives the same scores.  No atomics anywhere; every
// reduction has a fixed order.
#include "tpg_internal.h"
#include "../../include/tpgan.h"
#include <math.h>

namespace tpg {
namespace {

typedef __attribute__((ext_vector_type(16))) float mf32x16;

constexpr int ID_MAXD = 4096;
constexpr int ID_MAXROWS = 1 << 24;
constexpr int CT_ROWS = 128;        // probes per block, and gallery rows per tile
constexpr int CT_K = 32;            // depth staged per step
constexpr int CT_LD = CT_K + 4;     // LDS row stride in floats
constexpr int CT_SLOTS = 8;         // list length kept in registers (k <= 8)
constexpr int CT_EMPTY = 0x7fffffff;

struct Cand {
  float s;
  int32_t i;
};

// ---------------------------------------------------------------- rows of a strided view

template <typename E> __device__ __forceinline__ float ld_elem(const E* p) { return (float)*p; }

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }  // false for NaN

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

struct NormArgs {
  const void* x;
  int64_t s0, s1;
  float* out;
  float* norm;
  int32_t* status;
  int32_t n, d, dpad;
};

template <typename E>
__global__ __launch_bounds__(256) void l2_normalize_kernel(const NormArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.n) return;
  const E* x = reinterpret_cast<const E*>(a.x) + row * a.s0;
  float ss = 0.f;
  bool bad = false;
  for (int e = lane; e < a.d; e += 64) {
    const float v = ld_elem<E>(x + (int64_t)e * a.s1);
    bad |= !finite_f(v);
    ss = fmaf(v, v, ss);
  }
  ss = wave_sum(ss);
  bad = __any(bad) || !finite_f(ss) || ss == 0.f;
  const float nrm = sqrtf(ss);
  float* o = a.out + row * a.dpad;
  for (int e = lane; e < a.dpad; e += 64) {
    float v = 0.f;
    if (!bad && e < a.d) v = ld_elem<E>(x + (int64_t)e * a.s1) / nrm;
    o[e] = v;
  }
  if (lane == 0) {
    if (a.norm) a.norm[row] = nrm;
    a.status[row] = bad ? 1 : 0;
  }
}

struct PairArgs {
  const void* a;
  const void* b;
  int64_t a0, a1, b0, b1;
  float* cos;
  int32_t* status;
  int32_t n, d;
};

template <typename EA, typename EB>
__global__ __launch_bounds__(256) void cosine_pairs_kernel(const PairArgs p) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.n) return;
  const EA* a = reinterpret_cast<const EA*>(p.a) + row * p.a0;
  const EB* b = reinterpret_cast<const EB*>(p.b) + row * p.b0;
  float ab = 0.f, aa = 0.f, bb = 0.f;
  bool bad = false;
  for (int e = lane; e < p.d; e += 64) {
    const float u = ld_elem<EA>(a + (int64_t)e * p.a1), v = ld_elem<EB>(b + (int64_t)e * p.b1);
    bad |= !finite_f(u) || !finite_f(v);
    ab = fmaf(u, v, ab);
    aa = fmaf(u, u, aa);
    bb = fmaf(v, v, bb);
  }
  ab = wave_sum(ab);
  aa = wave_sum(aa);
  bb = wave_sum(bb);
  bad = __any(bad) || !finite_f(aa) || !finite_f(bb) || aa == 0.f || bb == 0.f;
  if (lane == 0) {
    p.cos[row] = bad ? 0.f : ab / (sqrtf(aa) * sqrtf(bb));
    p.status[row] = bad ? 1 : 0;
  }
}

// ---------------------------------------------------------------- cosine top-k

// score descending, ties to the lower gallery index; an empty slot (-inf, CT_EMPTY) loses to all
__device__ __forceinline__ bool better(float s, int i, float s2, int i2) { return s > s2 || (s == s2 && i < i2); }

struct TopList {
  float s[CT_SLOTS];
  int32_t i[CT_SLOTS];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < CT_SLOTS; ++j) s[j] = -INFINITY, i[j] = CT_EMPTY;
  }
  __device__ __forceinline__ void insert(float v, int g) {
#pragma unroll
    for (int j = CT_SLOTS - 1; j > 0; --j) {
      const bool up = better(v, g, s[j - 1], i[j - 1]), here = better(v, g, s[j], i[j]);
      s[j] = up ? s[j - 1] : (here ? v : s[j]);
      i[j] = up ? i[j - 1] : (here ? g : i[j]);
    }
    const bool here = better(v, g, s[0], i[0]);
    s[0] = here ? v : s[0];
    i[0] = here ? g : i[0];
  }
};

struct TopkArgs {
  const float* probes;
  const float* gallery;
  const int32_t* skip;
  Cand* part;       // [nchunks][P][k]
  int32_t* idx;
  float* score;
  int32_t P, G, dpad, k, ptiles, ksteps, nchunks;
  int64_t chunk;
};

__global__ __launch_bounds__(256) void cosine_topk_kernel(const TopkArgs a) {
  __shared__ __attribute__((aligned(16))) float sg[CT_ROWS * CT_LD];
  __shared__ __attribute__((aligned(16))) float sp[CT_ROWS * CT_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const int pt = blockIdx.x % a.ptiles, c = blockIdx.x / a.ptiles;
  const int p0 = pt * CT_ROWS;
  const int64_t gbeg64 = (int64_t)c * a.chunk;
  const int gbeg = (int)gbeg64;
  const int gend = (int)(gbeg64 + a.chunk < (int64_t)a.G ? gbeg64 + a.chunk : (int64_t)a.G);
  const int tiles = (gend - gbeg + CT_ROWS - 1) / CT_ROWS;
  const int nit = tiles * a.ksteps;

  // staging: 8 threads per row (32 floats), 32 rows per pass, 4 passes per operand
  const int srow = tid >> 3, sseg = (tid & 7) * 4;
  float4 rg[4], rp[4];
  auto fetch = [&](int it) {
    const int tile = it / a.ksteps, ks = it - tile * a.ksteps;
    const int kk = ks * CT_K + sseg;
    const int g0 = gbeg + tile * CT_ROWS;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int g = g0 + srow + 32 * j, p = p0 + srow + 32 * j;
      rg[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      rp[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (kk < a.dpad && g < gend) rg[j] = *reinterpret_cast<const float4*>(a.gallery + (int64_t)g * a.dpad + kk);
      if (kk < a.dpad && p < a.P) rp[j] = *reinterpret_cast<const float4*>(a.probes + (int64_t)p * a.dpad + kk);
    }
  };

  const int p = p0 + 32 * wave + lr;  // this lane's probe
  const int sk = (a.skip && p < a.P) ? a.skip[p] : -1;
  TopList top;
  top.clear();
  mf32x16 acc[4];

  if (nit > 0) fetch(0);
  for (int it = 0; it < nit; ++it) {
    __syncthreads();  // the previous step's reads are done
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      *reinterpret_cast<float4*>(&sg[(srow + 32 * j) * CT_LD + sseg]) = rg[j];
      *reinterpret_cast<float4*>(&sp[(srow + 32 * j) * CT_LD + sseg]) = rp[j];
    }
    __syncthreads();
    if (it + 1 < nit) fetch(it + 1);
    const int tile = it / a.ksteps, ks = it - tile * a.ksteps;
    if (ks == 0) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    }
    // lane half lh feeds k = 8q + 4lh + e of both operands to MFMA (q, e): each k once
#pragma unroll
    for (int q = 0; q < CT_K / 8; ++q) {
      if (ks * CT_K + 8 * q >= a.dpad) break;  // (uniform) nothing but zero columns left
      const float4 b = *reinterpret_cast<const float4*>(&sp[(32 * wave + lr) * CT_LD + 8 * q + 4 * lh]);
      float4 av[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) av[t] = *reinterpret_cast<const float4*>(&sg[(32 * t + lr) * CT_LD + 8 * q + 4 * lh]);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].x, b.x, acc[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].y, b.y, acc[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].z, b.z, acc[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].w, b.w, acc[t], 0, 0, 0);
    }
    if (ks == a.ksteps - 1) {
      // C layout: column (probe) = lane & 31, row (gallery) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
      // A lane meets its gallery rows in rising order, so an equal score never displaces an entry.
      const int gt = gbeg + tile * CT_ROWS + 4 * lh;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int g = gt + 32 * t + (r & 3) + 8 * (r >> 2);
          const float v = acc[t][r];
          if (v > top.s[CT_SLOTS - 1] && g < gend && g != sk) top.insert(v, g);
        }
    }
  }
  // the other half of this probe's rows
  float os[CT_SLOTS];
  int32_t oi[CT_SLOTS];
#pragma unroll
  for (int j = 0; j < CT_SLOTS; ++j) {
    os[j] = __shfl_xor(top.s[j], 32, 64);
    oi[j] = __shfl_xor(top.i[j], 32, 64);
  }
#pragma unroll
  for (int j = 0; j < CT_SLOTS; ++j) top.insert(os[j], oi[j]);
  if (lh == 0 && p < a.P) {
    Cand* o = a.part + ((int64_t)c * a.P + p) * a.k;
#pragma unroll
    for (int j = 0; j < CT_SLOTS; ++j)
      if (j < a.k) {
        Cand e;
        e.s = top.s[j];
        e.i = top.i[j];
        o[j] = e;
      }
  }
}

__global__ __launch_bounds__(256) void cosine_merge_kernel(const TopkArgs a) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.P) return;
  TopList top;
  top.clear();
  for (int c = 0; c < a.nchunks; ++c) {
    const Cand* in = a.part + ((int64_t)c * a.P + p) * a.k;
    for (int j = 0; j < a.k; ++j) {
      const Cand e = in[j];
      if (e.i == CT_EMPTY) break;  // lists are sorted: the rest is empty
      top.insert(e.s, e.i);
    }
  }
#pragma unroll
  for (int j = 0; j < CT_SLOTS; ++j)
    if (j < a.k) {
      a.idx[p * a.k + j] = top.i[j] == CT_EMPTY ? -1 : top.i[j];
      a.score[p * a.k + j] = top.s[j];
    }
}

// ---------------------------------------------------------------- host side

struct TopkPlan {
  int64_t chunk;
  int32_t nchunks, ptiles;
  int64_t ws_bytes;
};

int topk_plan(const char* fn, int32_t P, int32_t G, int32_t k, int32_t gchunk, TopkPlan* out) {
  if (P < 0 || P > ID_MAXROWS || G < 0 || G > ID_MAXROWS)
    return fail(-2, "%s: P and G must be in 0..2^24, got %d and %d", fn, P, G);
  if (k < 1 || k > CT_SLOTS) return fail(-2, "%s: k must be in 1..8, got %d", fn, k);
  if (gchunk < 0 || (gchunk >= 1 && gchunk <= 15))
    return fail(-2, "%s: gchunk must be 0 (automatic) or >= 16, got %d", fn, gchunk);
  const int64_t ptiles = P > 0 ? ((int64_t)P + CT_ROWS - 1) / CT_ROWS : 1;
  int64_t chunk = gchunk;
  if (gchunk == 0) {
    // about 1024 blocks (four per CU) where the gallery allows, whole tiles per chunk
    const int64_t tiles = G > 0 ? ((int64_t)G + CT_ROWS - 1) / CT_ROWS : 1;
    int64_t want = (1024 + ptiles - 1) / ptiles;
    if (want > tiles) want = tiles;
    chunk = (tiles + want - 1) / want * CT_ROWS;
  }
  const int64_t nchunks = ((int64_t)G + chunk - 1) / chunk;
  if (ptiles * nchunks > 0x7fffffffLL)
    return fail(-2, "%s: too many blocks (probe tiles x chunks >= 2^31); raise gchunk", fn);
  out->chunk = chunk;
  out->nchunks = (int32_t)nchunks;
  out->ptiles = (int32_t)ptiles;
  const int64_t bytes = (int64_t)sizeof(Cand) * P * nchunks * k;
  out->ws_bytes = bytes > 8 ? bytes : 8;
  return 0;
}

int rows_check(const char* fn, int32_t n, int32_t d) {
  if (n < 0 || n > ID_MAXROWS) return fail(-2, "%s: n must be in 0..2^24, got %d", fn, n);
  if (d < 1 || d > ID_MAXD) return fail(-2, "%s: d must be in 1..4096, got %d", fn, d);
  return 0;
}

bool dtype_ok(int32_t dt) { return dt == TPG_F32 || dt == TPG_BF16 || dt == TPG_F16; }

template <typename EA>
void launch_pairs(int32_t bdt, const PairArgs& p, dim3 grid, hipStream_t st) {
  if (bdt == TPG_F32) hipLaunchKernelGGL((cosine_pairs_kernel<EA, float>), grid, dim3(256), 0, st, p);
  else if (bdt == TPG_BF16) hipLaunchKernelGGL((cosine_pairs_kernel<EA, __bf16>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((cosine_pairs_kernel<EA, _Float16>), grid, dim3(256), 0, st, p);
}

}  // namespace
}  // namespace tpg

using namespace tpg;

extern "C" int32_t tpg_l2_normalize(int32_t n, int32_t d, tpg_tensor x, float* out, int32_t dpad, float* norm,
                                    int32_t* status, tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  const int rc = rows_check("l2_normalize", n, d);
  if (rc) return rc;
  if (dpad != (d + 3) / 4 * 4) return fail(-2, "l2_normalize: dpad must be d rounded up to a multiple of 4");
  if (!dtype_ok(x.dtype)) return fail(-3, "l2_normalize: bad dtype");
  if (n == 0) return 0;
  if (!x.data || !out || !status) return fail(-10, "l2_normalize: NULL pointer");
  NormArgs a;
  a.x = x.data;
  a.s0 = x.stride[0];
  a.s1 = x.stride[1];
  a.out = out;
  a.norm = norm;
  a.status = status;
  a.n = n;
  a.d = d;
  a.dpad = dpad;
  const dim3 grid((unsigned)((n + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
  if (x.dtype == TPG_F32) hipLaunchKernelGGL(l2_normalize_kernel<float>, grid, dim3(256), 0, st, a);
  else if (x.dtype == TPG_BF16) hipLaunchKernelGGL(l2_normalize_kernel<__bf16>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(l2_normalize_kernel<_Float16>, grid, dim3(256), 0, st, a);
  return launched("l2_normalize");
}

extern "C" int32_t tpg_cosine_pairs(int32_t n, int32_t d, tpg_tensor a, tpg_tensor b, float* cos, int32_t* status,
                                    tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  const int rc = rows_check("cosine_pairs", n, d);
  if (rc) return rc;
  if (!dtype_ok(a.dtype) || !dtype_ok(b.dtype)) return fail(-3, "cosine_pairs: bad dtype");
  if (n == 0) return 0;
  if (!a.data || !b.data || !cos || !status) return fail(-10, "cosine_pairs: NULL pointer");
  PairArgs p;
  p.a = a.data;
  p.b = b.data;
  p.a0 = a.stride[0];
  p.a1 = a.stride[1];
  p.b0 = b.stride[0];
  p.b1 = b.stride[1];
  p.cos = cos;
  p.status = status;
  p.n = n;
  p.d = d;
  const dim3 grid((unsigned)((n + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
  if (a.dtype == TPG_F32) launch_pairs<float>(b.dtype, p, grid, st);
  else if (a.dtype == TPG_BF16) launch_pairs<__bf16>(b.dtype, p, grid, st);
  else launch_pairs<_Float16>(b.dtype, p, grid, st);
  return launched("cosine_pairs");
}

extern "C" int64_t tpg_cosine_topk_workspace(int32_t P, int32_t G, int32_t k, int32_t gchunk) {
  TopkPlan pl;
  const int rc = topk_plan("cosine_topk_workspace", P, G, k, gchunk, &pl);
  return rc ? rc : pl.ws_bytes;
}

extern "C" int32_t tpg_cosine_topk(int32_t P, int32_t G, int32_t d, int32_t dpad, const float* probes,
                                   const float* gallery, int32_t k, const int32_t* skip, int32_t gchunk, int32_t* idx,
                                   float* score, void* ws, size_t ws_bytes, tpg_stream_t stream) {
  if (int32_t grc = group_sync()) return grc;
  TopkPlan pl;
  int rc = topk_plan("cosine_topk", P, G, k, gchunk, &pl);
  if (rc) return rc;
  if (d < 1 || d > ID_MAXD) return fail(-2, "cosine_topk: d must be in 1..4096");
  if (dpad != (d + 3) / 4 * 4) return fail(-2, "cosine_topk: dpad must be d rounded up to a multiple of 4");
  if (P == 0) return 0;
  if (!probes || (G > 0 && !gallery) || !idx || !score || !ws) return fail(-10, "cosine_topk: NULL pointer");
  if ((uintptr_t)probes % 16 != 0 || (uintptr_t)gallery % 16 != 0 || (uintptr_t)ws % 8 != 0)
    return fail(-4, "cosine_topk: probes and gallery must be 16-byte aligned, the workspace 8-byte aligned");
  if ((int64_t)ws_bytes < pl.ws_bytes)
    return fail(-4, "cosine_topk: workspace too small (tpg_cosine_topk_workspace)");
  TopkArgs a;
  a.probes = probes;
  a.gallery = gallery;
  a.skip = skip;
  a.part = reinterpret_cast<Cand*>(ws);
  a.idx = idx;
  a.score = score;
  a.P = P;
  a.G = G;
  a.dpad = dpad;
  a.k = k;
  a.ptiles = pl.ptiles;
  a.ksteps = (dpad + CT_K - 1) / CT_K;
  a.nchunks = pl.nchunks;
  a.chunk = pl.chunk;
  hipStream_t st = (hipStream_t)stream;
  if (pl.nchunks > 0) {
    hipLaunchKernelGGL(cosine_topk_kernel, dim3((unsigned)((int64_t)pl.ptiles * pl.nchunks)), dim3(256), 0, st, a);
    rc = launched("cosine_topk");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(cosine_merge_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, a);
  return launched("cosine_topk");
}
