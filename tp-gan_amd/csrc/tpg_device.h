// Device helpers shared by the conv kernel files (tpg_igemm / tpg_halo / tpg_pw / tpg_wgrad /
// tpg_wgrad2 / tpg_wgrad_rh .hip) and the weight packers: vector types, the reflect index, the LDS
// chunk swizzles with the one transposed-read wrapper, the pack items that write the swizzled
// weight image, and the output / residual offsets of a pixel.  Everything is
// __device__ __forceinline__: no kernel, no state.
#pragma once
#include "tpg_internal.h"

namespace tpg {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

// reflect padding: the mirrored index of i in [0, n) (|i| and 2n - 2 - i: one fold each side)
__device__ __forceinline__ int tpg_refl(int i, int n) {
  i = i < 0 ? -i : i;
  return i >= n ? 2 * n - 2 - i : i;
}

// ---------------------------------------------------------------- LDS chunk swizzles ----
// Each returns the XOR mask of the 16-byte chunk index inside an LDS row: chunk c of row `row`
// is stored at c ^ swz(row), and readers XOR back.
//
// 64-byte rows read whole by ds_read_b128 (the halo and pointwise kernels' pixel and weight
// rows): conflict-free fragment reads of both operands for any tap shift (checked exhaustively
// over the gfx950 ds_read_b128 lane groups).  The packed halo weight image is stored with this
// mask (pack_halo_item, pack_halo_block_t), the halo kernel's fragment reads and the pointwise
// kernel's choice of each lane's DMA source chunk undo it: all through this one function.
__device__ __forceinline__ int swz64(int row) { return ((row >> 2) & 1) << 1; }

// 16-bit rows of ROW_BYTES read transposed (ds_read_b64_tr_b16, the weight-gradient kernels): a
// read takes, per 32-lane half, 32-byte pieces of 8 rows {R .. R + 3, R + 8 .. R + 11}; the mask
// puts the 8 pieces on 8 different chunk pairs of a 256-byte bank row.  256-byte rows: every row
// is one bank row, so bits 0-1 and 3 of the row spread the pieces; 128-byte rows: bit 0 of the
// row already selects the bank-row half, bits 1 and 3 do the rest; 64-byte rows: bits 0-1 select
// the quarter, bit 3 keeps the two row quads (the g = 0 / 1 octets) on disjoint chunk pairs.
// (Not swz64: that one reads bit 2, the b128 lane groups' row bit.)
template <int ROW_BYTES>
__device__ __forceinline__ int tr_swz(int row) {
  static_assert(ROW_BYTES == 256 || ROW_BYTES == 128 || ROW_BYTES == 64, "row sizes with a conflict analysis");
  if constexpr (ROW_BYTES == 256) return ((row & 3) | (((row >> 3) & 1) << 2)) << 1;
  else if constexpr (ROW_BYTES == 128) return (((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 1;
  else return ((row >> 3) & 1) << 1;
}
// fp32 rows read by ds_read_b32 (the parity mode of tpg_wgrad / tpg_wgrad2): a read takes 2 rows
// per 32-lane half
__device__ __forceinline__ int f32_swz(int row) { return (row & 1) << 2; }

// ds_read_b64_tr_b16 at LDS byte address a (+ off in the instruction's offset field: a constant
// once the caller's loops are unrolled).  Inline asm: a builtin LDS read makes hipcc put
// s_waitcnt vmcnt(0) in front of it for the LDS-DMA in flight (+18 % on the 256 x 32 row-halo
// tile); the callers count their own lgkmcnt waits.
__device__ __forceinline__ s16x4 tr_read(uint32_t a, int off = 0) {
  s16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(a), "i"(off));
  return v;
}

// ---------------------------------------------------------------- weight pack items ----
// igemm layout: item = (n', unit) -> 16 consecutive elements of Wp row n'
template <typename E>
__device__ __forceinline__ void pack_igemm_item(const PackArgs& p, int idx) {
  const int np = idx / p.nunits;
  const int unit = idx - np * p.nunits;
  const int tap = unit / p.upt;
  const int cbase = (unit - tap * p.upt) * 16;
  E out[16];
  const bool ok = np < p.Nreal && tap < p.ntaps;
  int a = 0, b = 0, r = ok ? p.tr[tap] : 0, s = ok ? p.ts[tap] : 0;
  if (p.nmode == 0) a = np;
  else if (p.nmode == 1) b = np;
  else {
    const int rs = np / p.comp_c, ch = np - rs * p.comp_c;
    r = rs / p.comp_kw; s = rs - r * p.comp_kw;
    if (p.nmode == 2) b = ch; else a = ch;
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int cp = cbase + e;
    float v = 0.f;
    if (ok && cp < p.Creal) {
      int aa = a, bb = b, rr = r, ss = s;
      if (p.cmode == 0) aa = cp;
      else if (p.cmode == 1) bb = cp;
      else {
        const int rs = cp / p.comp_c, ch = cp - rs * p.comp_c;
        rr = rs / p.comp_kw; ss = rs - rr * p.comp_kw;
        if (p.cmode == 2) bb = ch; else aa = ch;
      }
      v = p.W[(int64_t)aa * p.w_sa + (int64_t)bb * p.w_sb + (int64_t)rr * p.w_sr + (int64_t)ss * p.w_ss];
    }
    out[e] = (E)v;
  }
  uint4* dst = reinterpret_cast<uint4*>(reinterpret_cast<E*>(p.Wp) + (int64_t)idx * 16);
  const uint4* src = reinterpret_cast<const uint4*>(out);
#pragma unroll
  for (int q = 0; q < (int)(16 * sizeof(E) / 16); ++q) dst[q] = src[q];
}

// halo layout: Wp[ks*ntaps + tap][ntile][bnl rows][4 chunks][EPC]; item = one 16-byte chunk;
// row r of N-tile nt is n' = nt*bn + r, chunk' = chunk ^ swz64(r)
template <typename E>
__device__ __forceinline__ void pack_halo_item(const PackArgs& p, int bn, int bnl, int ntiles, int idx) {
  constexpr int EPC = 16 / sizeof(E);
  constexpr int ROW = 4 * EPC;
  const int pchunk = idx & 3;
  int rr = idx >> 2;
  const int r = rr % bnl;
  rr /= bnl;
  const int nt = rr % ntiles;
  rr /= ntiles;
  // step rr: k-step rr / ntaps, tap rr % ntaps; past the full k-steps of a paired image (half:
  // the last k-step holds <= 16 live channels) step j carries taps 2j (logical chunks 0, 1) and
  // 2j + 1 (chunks 2, 3), channels 0..15 of that k-step each (tpg_halo.hip compute)
  const int lc = pchunk ^ swz64(r);
  const int nfull = (p.half ? p.hnks - 1 : p.hnks) * p.ntaps;
  int tap, c0;
  bool tap_ok = true;
  if (rr < nfull) {
    tap = rr % p.ntaps;
    c0 = (rr / p.ntaps) * ROW + lc * EPC;
  } else {
    tap = 2 * (rr - nfull) + (lc >> 1);
    c0 = (p.hnks - 1) * ROW + (lc & 1) * EPC;
    tap_ok = tap < p.ntaps;
    if (!tap_ok) tap = 0;
  }
  const int np = nt * bn + r;
  union { uint4 u; E e[EPC]; } o;
  const bool row_ok = r < bn && np < p.Nreal && tap_ok;
  const int tr = p.tr[tap], ts = p.ts[tap];
  const int64_t base = (int64_t)tr * p.w_sr + (int64_t)ts * p.w_ss +
                       (p.nmode == 0 ? (int64_t)np * p.w_sa : (int64_t)np * p.w_sb);
  const int64_t cstride = p.cmode == 0 ? p.w_sa : p.w_sb;
  const float* src = p.W + base + (int64_t)c0 * cstride;
  if (cstride == 1 && row_ok && c0 + EPC <= p.Creal && ((uintptr_t)src % 16) == 0) {
    // contiguous input channels (the forward images of channels-last weights): 16-byte loads
#pragma unroll
    for (int q = 0; q < EPC / 4; ++q) {
      const float4 v = reinterpret_cast<const float4*>(src)[q];
      o.e[4 * q] = (E)v.x; o.e[4 * q + 1] = (E)v.y; o.e[4 * q + 2] = (E)v.z; o.e[4 * q + 3] = (E)v.w;
    }
  } else if (cstride == 1 && row_ok && c0 + EPC <= p.Creal && ((uintptr_t)src % 8) == 0) {
    // (an even channel count that is not a multiple of 4 -- 206 -- leaves every other tap's
    // rows 8-byte aligned only: 8-byte loads instead of 4-byte ones; G's re-pack 0.489 ->
    // 0.470 ms, tools/bench_opt.py, gpurun r06r)
#pragma unroll
    for (int q = 0; q < EPC / 2; ++q) {
      const float2 v = reinterpret_cast<const float2*>(src)[q];
      o.e[2 * q] = (E)v.x; o.e[2 * q + 1] = (E)v.y;
    }
  } else {
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
      const int c = c0 + e;
      o.e[e] = (E)((row_ok && c < p.Creal) ? p.W[base + (int64_t)c * cstride] : 0.f);
    }
  }
  reinterpret_cast<uint4*>(p.Wp)[idx] = o.u;
}

// ---------------------------------------------------------------- output offsets ----
// Element offsets of output pixel (nimg, j, i) of the (sub-)grid in Y (.y) and in the residual R
// (.r); IgemmArgs, HaloArgs and EpiArgs share the field names.  (Returned by value: with pointer
// outputs the halo kernel's row-table code came out in another order.)
struct OutOff { int64_t y, r; };
template <typename A>
__device__ __forceinline__ OutOff out_offsets(const A& p, int nimg, int j, int i) {
  const int oy = p.oy0 + p.osy * j, ox = p.ox0 + p.osx * i;
  return {(int64_t)nimg * p.y_sn + (int64_t)oy * p.y_sh + (int64_t)ox * p.y_sw,
          (int64_t)nimg * p.r_sn + (int64_t)oy * p.r_sh + (int64_t)ox * p.r_sw};
}

}  // namespace tpg
