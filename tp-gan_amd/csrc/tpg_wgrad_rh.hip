// Weight gradient of a stride-1 Conv2d by kernel-row halos (gfx950, bf16):
//   dW[a][b][r][s] += sum_{n,py,px} dY[n][py][px][a] * X[n][py + r - pt][px + s - pl][b].
//
// tpg_wgrad2.hip flattens (tap, b) into GEMM columns, so every 64-pixel k-tile DMAs the dY
// tile once per 128-column tile and the X pixels once per TAP: for a 5x5 206-channel layer
// at 128x128 that is ~16 GB of LDS-DMA per call and the kernel runs at the chip's DMA-fill
// rate, not the MFMA rate.  Here a block owns one kernel row r and a group of NT horizontal
// taps s0..s0+NT-1 (GEMM columns = NT x 64 channels), and a k-tile is 64 consecutive
// pixels of ONE image row, so the X operand of all NT taps is a single row segment of
// 64 + NT - 1 halo pixels, loaded once; tap s reads it shifted by s rows in LDS.  Bytes per
// flop drop ~2.4x (dY 16 KB + X 9 KB per 5.2 MFLOP at NT = 5).
//
// Pipeline as in wgrad2: 8 waves, both operands by buffer LDS-DMA (out-of-range offsets read
// zero = padding), 3-stage ring two k-tiles ahead, one counted vmcnt + barrier per k-tile,
// ds_read_b64_tr_b16 fragment reads for v_mfma_f32_16x16x32_bf16, fp32 atomics over the
// pixel splits.  Blocks of one pixel split are adjacent in the XCD-aware order, so the
// tiles that read the same dY / X rows run together on one XCD's L2.
#include "tpg_device.h"
#include <type_traits>
#include <utility>

// timing ablations (tools only; never in the product build): bit 1 no LDS-DMA, 2 no barrier,
// 4 no MFMA, 8 no fragment reads
#ifndef TPG_RH_ABL
#define TPG_RH_ABL 0
#endif

namespace tpg {

// The tiles held to 128 VGPRs (two 512-thread blocks per CU)
template <int NR, int NT, int BM, int BC>
constexpr bool rh_fits128() {
  return NR == 2 || (NR == 1 && ((BM == 128 && BC == 32 && NT <= 5) || (BM == 64 && BC == 64 && NT <= 4) ||
                                 (BM == 64 && BC == 32)));
}

// XCD-aware block order: physical block b runs on XCD b % 8 and each XCD is handed a contiguous
// range of logical blocks (this block's is returned)
__device__ __forceinline__ int xcd_logical_block() {
  const int nblk = gridDim.x, full = nblk & ~7, bid = blockIdx.x;
  return bid < full ? (bid & 7) * (full >> 3) + (bid >> 3) : bid;
}
// buffer resource of a DMA operand: offsets at or past `bytes` read zero
__device__ __forceinline__ __amdgpu_buffer_rsrc_t dma_rsrc(const void* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}

// dynamic LDS of wgrad_rh_kernel: three stages of 64 dY rows and the X halo in whole rounds of
// eight 1 KiB pieces
template <int NR, int BM, int BC>
constexpr int rh_lds_bytes() { return 3 * (64 * BM * 2 + ((NR == 1 ? 72 : 200) * BC * 2 + 8191) / 8192 * 8192); }

template <int DT, int NR, int NT, int BM, int BC>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(rh_fits128<NR, NT, BM, BC>() ? 4 : 1)))
void wgrad_rh_kernel(const WgradRHArgs p) {
  // k-tile: 64 pixels = TH x TW (TW = p.tw: a row segment of 64, or TH = 64 / TW whole rows of
  // a narrower map); block taps: NR kernel rows x NT columns (row mode NR = 1, image mode
  // NR = kh), all read from one (TH + NR - 1) x (TW + NT - 1) X halo of the k-tile
  constexpr int KP = 64;
  // BM a (dY channels) x BC b (X channels) per block; GEMM columns: (tap, b)
  constexpr int BN = NR * NT * BC;
  constexpr int WM = (BM == 64 && BC == 64) ? 2 : 4, WN = 8 / WM;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int MREP = WTM / 16, NREP = WTN / 16;
  constexpr int RBA = BM * 2, RBB = BC * 2;  // LDS row bytes
  // row size whose chunk swizzle the dY rows take (tr_swz, tpg_device.h; the X rows: RBB).  The
  // 256-channel tile's 512-byte rows have always taken the 64-byte rows' mask -- the former
  // three-way branch fell through to it -- which leaves the four rows R .. R + 3 of a transposed
  // read on one chunk pair; kept bit for bit (the 256-byte mask is the candidate, to be timed)
  constexpr int SWA = RBA == 512 ? 64 : RBA;
  constexpr int BYTES_A = KP * RBA;
  constexpr int GA = BYTES_A / 8192;         // 1 KiB DMA pieces per wave for dY
  constexpr int HROWS = NR == 1 ? 72 : 200;  // >= (TH + NR - 1) * (TW + NT - 1) halo pixels
  constexpr int BYTES_B = HROWS * RBB;
  constexpr int PB = (BYTES_B + 1023) / 1024, GB = (PB + 7) / 8;  // X pieces, per wave
  constexpr int RPP = 1024 / RBA, RPB = 1024 / RBB;              // rows per piece
  constexpr int STAGE = BYTES_A + GB * 8 * 1024;
  static_assert(NR == 1 ? ((NT >= 3 && NT <= 5) || NT == 7) : (NR == NT && NT <= 3), "taps per block");
  static_assert(GA * 8192 == BYTES_A && GA >= 1 && GB <= 2, "dma pieces");
  static_assert(3 * STAGE == rh_lds_bytes<NR, BM, BC>(), "the launcher's LDS size");
  static_assert(MREP * 16 * WM == BM && NREP * 16 * WN == BN, "waves");

  extern __shared__ __attribute__((aligned(16))) char lds[];  // [3][STAGE]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

  const int L = xcd_logical_block();  // = split * tiles + tile
  const int tile = L % p.tiles, split = L / p.tiles;
  int t = tile;
  const int ta = t % p.nta; t /= p.nta;
  const int tb = t % p.ntb; t /= p.ntb;
  const int r0 = (t % p.nrg) * NR;
  const int s0 = (t / p.nrg) * NT;
  const int a0 = ta * BM, b0 = tb * BC;
  const int kt0 = split * p.kt_per_split;
  const int nkt = min(p.nkt, kt0 + p.kt_per_split) - kt0;
  if (nkt <= 0) return;
  // bias gradient: the blocks of the first b tile, kernel row group and tap group see every
  // dY pixel of their split exactly once; one wave column of them sums the A fragments
  // (k-tile kt of the split is summed by the tile with share index kt % bshare, so the extra
  // MFMAs spread evenly over the a-tile's blocks; bshare = 1 keeps one owner: deterministic)
  const int sid = tb + p.ntb * (t % p.nrg + p.nrg * (t / p.nrg));
  const bool has_bias = p.dbias != nullptr && sid < p.bshare;

  // position of k-tile kt0: (n, py, px0), advanced incrementally (all scalar)
  // TH = floor(64 / TW): pixels TH*TW..63 of a k-tile are dead (zero dY rows), and a last
  // band may run past the map (its rows read zero as well)
  const int TW = p.tw, TH = KP / TW, HW = TW + NT - 1;
  const int segs = p.PW / TW, bands = (p.PH + TH - 1) / TH;
  int n = kt0 / (bands * segs);
  int rem = kt0 - n * bands * segs;
  int py = (rem / segs) * TH;
  int px0 = (rem % segs) * TW;

  const __amdgpu_buffer_rsrc_t rP = dma_rsrc(p.P, p.p_bytes), rQ = dma_rsrc(p.Q, p.q_bytes);
  constexpr unsigned OOB = 0x80000000u;

  // per-lane constants of the DMA pieces
  //   dY piece j of wave w: tile rows (GA*w + j) * RPP .. +RPP-1
  unsigned aoff[GA];
  int ary[GA];  // pixel row of the dY tile row inside the k-tile (large = dead)
#pragma unroll
  for (int j = 0; j < GA; ++j) {
    const int row = (wave * GA + j) * RPP + lane / (RBA / 16), pc = lane % (RBA / 16);
    const int c = a0 + ((pc ^ tr_swz<SWA>(row)) << 3);
    const bool live = c < p.Ca && row < TH * TW;
    aoff[j] = live ? (unsigned)(((row / TW) * p.p_sh + (row % TW) * p.p_sw + c) * 2) : OOB;
    ary[j] = live ? row / TW : (1 << 28);
  }
  //   X piece j * 8 + w: halo rows (j * 8 + w) * RPB ..; pieces past PB only pad the count
  const int nhalo = (TH + NR - 1) * HW;
  int bhy[GB], bhx[GB], bch[GB];
#pragma unroll
  for (int j = 0; j < GB; ++j) {
    const int row = (j * 8 + wave) * RPB + lane / (RBB / 16), pc = lane % (RBB / 16);
    const int c = b0 + ((pc ^ tr_swz<RBB>(row)) << 3);
    bhy[j] = row / HW + r0 - p.pt;             // + py  = X row of this halo pixel
    bhx[j] = row % HW + s0 - p.pl;             // + px0 = X column
    bch[j] = (c < p.Cb && row < nhalo && j * 8 + wave < PB) ? c : -1;
  }

  auto issue = [&](int slot, int n_, int py_, int px_) {
    if constexpr ((TPG_RH_ABL & 1) != 0) return;
    char* st = lds + slot * STAGE;
    const int sbase = (n_ * p.p_sn + py_ * p.p_sh + px_ * p.p_sw) * 2;
#pragma unroll
    for (int j = 0; j < GA; ++j) {
      // (a local copy: hipcc silently drops the kernel's host stub when the dependent-size
      // array element goes into the builtin directly)
      const unsigned vo = py_ + ary[j] < p.PH ? aoff[j] : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rP, (__attribute__((address_space(3))) void*)(st + (wave * GA + j) * 1024),
                                               16, vo, sbase, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < GB; ++j) {
      int qy = py_ + bhy[j], qx = px_ + bhx[j];
      bool ok = bch[j] >= 0;
      if (p.pad_mode) { qy = tpg_refl(qy, p.QH); qx = tpg_refl(qx, p.QW); }
      else ok = ok && (unsigned)qy < (unsigned)p.QH && (unsigned)qx < (unsigned)p.QW;
      const unsigned off = ok ? (unsigned)((n_ * p.q_sn + qy * p.q_sh + qx * p.q_sw + bch[j]) * 2) : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rQ, (__attribute__((address_space(3))) void*)(st + BYTES_A + (j * 8 + wave) * 1024),
                                               16, off, 0, 0, 0);
    }
  };

  const int wm = wave / WN, wn = wave % WN;
  // MFMA blocks of a padded edge tile that hold no real dW element -- 16 rows at or past Ca, or
  // 16 columns whose b channel is at or past Cb or whose tap is past the kernel -- read zeros;
  // their MFMAs are skipped (p.skip; wave-uniform masks, a scalar branch per MFMA).  206
  // channels pad to 256 rows x 224 columns per tap, a quarter of the MFMAs dead.
  unsigned mlive = ~0u, jlive = ~0u;
  if (p.skip) {
    mlive = 0;
    jlive = 0;
#pragma unroll
    for (int m = 0; m < MREP; ++m)
      if (a0 + wm * WTM + m * 16 < p.Ca) mlive |= 1u << m;
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
      const int col = wn * WTN + j * 16, tap = col / BC;
      if (b0 + col % BC < p.Cb && r0 + tap / NT < p.kh && s0 + tap % NT < p.kw) jlive |= 1u << j;
    }
    mlive = __builtin_amdgcn_readfirstlane(mlive);
    jlive = __builtin_amdgcn_readfirstlane(jlive);
  }
  const int g = lane >> 4, l16 = lane & 15;
  const int q = l16 >> 2, p4 = l16 & 3;
  const bool bias_wave = has_bias && wn == 0;
  f32x4 acc[MREP][NREP], accb[MREP];
#pragma unroll
  for (int m = 0; m < MREP; ++m) {
    accb[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NREP; ++j) acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const bf16x8 ones = __builtin_bit_cast(bf16x8, u32x4{one_pair<DT>(), one_pair<DT>(), one_pair<DT>(), one_pair<DT>()});

  // Fragment reads (transposed, 4 channels x 4 pixels per lane and read): fragment r < 2*MREP
  // is dY (A), the rest X halo rows shifted by the column's tap.  Next substep's reads are
  // issued between this substep's MFMAs (as in wgrad2).
  // Row mode: per-lane LDS byte offsets of the fragment reads.  The chunk swizzles depend on
  // the row only through bits the substep (+32 rows) and, for A, the K half (+4 rows) leave
  // alone, so every read is one of MREP + 2 * NREP lane offsets plus a constant (the
  // instruction's offset field): ~40 % fewer VALU in the k-tile loop.
  constexpr bool IMM = NR == 1;
  int abase[IMM ? MREP : 1], bbase[IMM ? NREP : 1][2];
  if constexpr (IMM) {
#pragma unroll
    for (int m = 0; m < MREP; ++m) {
      const int col = wm * WTM + m * 16 + 4 * p4, row = 8 * g + q;
      abase[m] = row * RBA + (((col >> 3) ^ tr_swz<SWA>(row)) << 4) + (col & 7) * 2;
    }
#pragma unroll
    for (int j = 0; j < NREP; ++j)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int col = wn * WTN + j * 16 + 4 * p4;
        const int tap = col / BC, cb = col % BC;
        const int row = 8 * g + 4 * h + q + tap;  // (row mode: halo row = pixel + tap)
        bbase[j][h] = BYTES_A + row * RBB + (((cb >> 3) ^ tr_swz<RBB>(row)) << 4) + (cb & 7) * 2;
      }
    // opaque to the optimiser: kept as one register each (rematerialised from their parts they
    // cost two VALU per read and k-tile)
#pragma unroll
    for (int m = 0; m < MREP; ++m) asm volatile("" : "+v"(abase[m]));
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
      asm volatile("" : "+v"(bbase[j][0]));
      asm volatile("" : "+v"(bbase[j][1]));
    }
  }
  // halo row of this lane's pixel k = ks*32 + 8g + 4h + q for tap (0, 0): (k / TW) * HW + k % TW
  int kbase[2][2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = ks * 32 + 8 * g + 4 * h + q;
      kbase[ks][h] = (k / TW) * HW + k % TW;
    }
  // BIAS (compile-time): the bias MFMAs sit beside the regular MFMA holding each A fragment
  // (see tpg_wgrad2.hip: no runtime branch inside this hand-scheduled region)
  auto compute = [&](int slot, bool bias_now) {
    const char* A = lds + slot * STAGE;
    const char* B = A + BYTES_A;
    constexpr int NS = KP / 32;
    constexpr int R = 2 * (MREP + NREP), M = MREP * NREP;
    auto addr = [&](int ks, int rr) -> const char* {
      if (rr < 2 * MREP) {
        const int col = wm * WTM + (rr >> 1) * 16 + 4 * p4;
        const int row = ks * 32 + 8 * g + 4 * (rr & 1) + q;
        return A + row * RBA + (((col >> 3) ^ tr_swz<SWA>(row)) << 4) + (col & 7) * 2;
      }
      const int r2 = rr - 2 * MREP;
      const int col = wn * WTN + (r2 >> 1) * 16 + 4 * p4;  // (tap, b) column
      const int tap = col / BC, cb = col % BC;
      const int row = kbase[ks][r2 & 1] + (tap / NT) * HW + tap % NT;
      return B + row * RBB + (((cb >> 3) ^ tr_swz<RBB>(row)) << 4) + (cb & 7) * 2;
    };
    // IMM: lane base + constant offset (asm: a builtin LDS read makes hipcc put vmcnt(0) in
    // front of it for the in-flight LDS-DMA, measured +18 % on the 256 x 32 tile)
    auto rd = [&](int ks, int rr) -> s16x4 {
      if constexpr (IMM) {
        if (rr < 2 * MREP) return tr_read(lds_addr(A + abase[rr >> 1]), (32 * ks + 4 * (rr & 1)) * RBA);
        const int r2 = rr - 2 * MREP;
        return tr_read(lds_addr(A + bbase[r2 >> 1][r2 & 1]), 32 * ks * RBB);
      } else {
        return tr_read(lds_addr(addr(ks, rr)));
      }
    };
    s16x4 h[2][R];
    // (first-use order, counted waits below: the MFMAs start on their own operands)
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int rr = frag_read_order<MREP, NREP>(k);
      if constexpr ((TPG_RH_ABL & 8) == 0) h[0][rr] = rd(0, rr);
      else h[0][rr] = s16x4{(short)lane, 1, 2, 3};
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < NS; ++ks) {
      const int cur = ks & 1;
#pragma unroll
      for (int i = 0; i < M; ++i) {
        const int m = i / NREP, j = i % NREP;
        if (ks == 0) {
          wait_lgkm(frag_read_wait<MREP, NREP>(i, i * R / M));
          __builtin_amdgcn_sched_barrier(0);
        }
        const bf16x8 av = __builtin_bit_cast(bf16x8, __builtin_shufflevector(h[cur][2 * m], h[cur][2 * m + 1],
                                                                             0, 1, 2, 3, 4, 5, 6, 7));
        const bf16x8 bv = __builtin_bit_cast(bf16x8, __builtin_shufflevector(h[cur][2 * MREP + 2 * j],
                                                                             h[cur][2 * MREP + 2 * j + 1],
                                                                             0, 1, 2, 3, 4, 5, 6, 7));
        if constexpr ((TPG_RH_ABL & 4) == 0) {
          if ((mlive >> m) & (jlive >> j) & 1u) acc[m][j] = mfma16x16x32<DT>(av, bv, acc[m][j]);
        }
        else acc[m][j][0] += (float)av[0] * (float)bv[1];
        if (ks + 1 < NS) {
#pragma unroll
          for (int rr = i * R / M; rr < (i + 1) * R / M; ++rr) {
            if constexpr ((TPG_RH_ABL & 8) == 0)
              h[cur ^ 1][rr] = rd(ks + 1, rr);
            else h[cur ^ 1][rr] = h[cur][rr];
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (ks + 1 < NS) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // bias (dY row sums) of an owned k-tile, after the hand-scheduled region: the A fragments
    // of both substeps are still in h (substep 1 read into h[1]) and every read has been
    // waited on.  (Bias MFMAs inside the region needed a second, compile-time copy of it,
    // which doubled its hoisted LDS addresses and spilled the wide tiles.)
    static_assert(NS == 2, "h holds both substeps");
    if (bias_now) {
    #pragma unroll
      for (int ks = 0; ks < NS; ++ks)
    #pragma unroll
        for (int m = 0; m < MREP; ++m)
          accb[m] = mfma16x16x32<DT>(__builtin_bit_cast(bf16x8, __builtin_shufflevector(h[ks][2 * m], h[ks][2 * m + 1],
                                                                                       0, 1, 2, 3, 4, 5, 6, 7)),
                                     ones, accb[m]);
    }
  };

  // pipeline: k-tile i in ring slot i % 3, issued two k-tiles ahead (clamped: static vmcnt)
  int in_ = n, iy = py, ix = px0, issued = 0;  // position of the next k-tile to issue
  auto issue_next = [&](int slot) {
    issue(slot, in_, iy, ix);
    if (++issued < nkt) {
      ix += TW;
      if (ix == p.PW) { ix = 0; iy += TH; if (iy >= p.PH) { iy = 0; ++in_; } }  // (partial last band)
    }
  };
#if (TPG_RH_ABL & 2) != 0
#define RH_WAIT_BARRIER() asm volatile("s_waitcnt vmcnt(6)\n\ts_waitcnt lgkmcnt(0)" ::: "memory")
#else
#define RH_WAIT_BARRIER() \
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::"n"(GA + GB) : "memory")
#endif
  static_assert(GA + GB >= 2 && GA + GB <= 6, "vmcnt");
  issue_next(0);
  issue_next(1);
  RH_WAIT_BARRIER();  // retires k-tile 0
  int slot = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    issue_next(slot == 0 ? 2 : slot - 1);
    compute(slot, bias_wave && (kt0 + kt) % p.bshare == sid);  // (one inlined copy)
    RH_WAIT_BARRIER();  // retires k-tile kt+1, kt+2 stays in flight
    slot = slot == 2 ? 0 : slot + 1;
  }
#undef RH_WAIT_BARRIER
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- epilogue through LDS, in row chunks that fit the ring (see tpg_wgrad2.hip): sole owner
  // (ksplit == 1) 16-byte read-add-write of 4 consecutive columns; pixel splits one no-return
  // atomic per lane with 64 lanes on 64 consecutive columns of one dW row (full-rate shape,
  // instead of the MFMA C layout's four 64-byte segments in four rows)
  constexpr int LDC = BN + 4;
  constexpr int RING = 3 * STAGE;
  constexpr int RCH0 = (RING / (LDC * 4)) / WTM * WTM;  // rows per chunk: whole wave rows
  constexpr int RCH = RCH0 < BM ? RCH0 : BM;
  static_assert(RCH >= WTM, "a wave row of the C tile fits in the LDS ring");
  float* Cs = reinterpret_cast<float*>(lds);
  const int amax = min(BM, p.Ca - a0);
  auto col_off = [&](int col) -> int {  // dW element offset of tile column col at a = 0; -1: padding
    const int tap = col / BC;
    const int r = r0 + tap / NT, s = s0 + tap % NT, b = b0 + col % BC;
    if (r >= p.kh || s >= p.kw || b >= p.Cb) return -1;
    return b * p.w_sb + r * p.w_sr + s * p.w_ss;
  };
  constexpr int CG = (BN + 63) / 64;
  int coff[CG];
#pragma unroll
  for (int c = 0; c < CG; ++c) coff[c] = (c * 64 + lane < BN) ? col_off(c * 64 + lane) : -1;
  const bool vec_base = p.w_sb == 1 && (p.w_sa & 3) == 0 && ((uintptr_t)p.dW & 15) == 0;
  asm volatile("s_barrier" ::: "memory");  // (every wave's DMAs retired above: the ring is free)
#pragma unroll
  for (int c0 = 0; c0 < BM; c0 += RCH) {
    if (c0 > 0) __syncthreads();  // the previous chunk has been read
    if (wm * WTM >= c0 && wm * WTM < c0 + RCH) {
#pragma unroll
      for (int m = 0; m < MREP; ++m)
#pragma unroll
        for (int j = 0; j < NREP; ++j)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg)
            Cs[(wm * WTM - c0 + m * 16 + 4 * g + reg) * LDC + wn * WTN + j * 16 + l16] = acc[m][j][reg];
    }
    __syncthreads();
    const int rows = min(RCH, amax - c0);
    if (p.ksplit == 1) {
      constexpr int CPR = BN / 4;
      for (int idx = tid; idx < rows * CPR; idx += 512) {
        const int row = idx / CPR, cc = 4 * (idx - row * CPR);
        const float4 v = *reinterpret_cast<const float4*>(Cs + row * LDC + cc);
        float* dst = p.dW + (a0 + c0 + row) * p.w_sa;
        const int o0 = col_off(cc);
        if (vec_base && o0 >= 0 && (o0 & 3) == 0 && col_off(cc + 3) == o0 + 3) {
          float4* d4 = reinterpret_cast<float4*>(dst + o0);
          float4 o = *d4;
          o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
          *d4 = o;
        } else {
          const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int oe = col_off(cc + e);
            if (oe >= 0) dst[oe] += vv[e];
          }
        }
      }
    } else {
      for (int row = wave; row < rows; row += 8) {
        float* dst = p.dW + (a0 + c0 + row) * p.w_sa;
#pragma unroll
        for (int c = 0; c < CG; ++c)
          if (coff[c] >= 0) atomicAdd(dst + coff[c], Cs[row * LDC + c * 64 + lane]);
      }
    }
  }
  if (bias_wave && l16 == 0) {  // every column of accb holds the row sum
#pragma unroll
    for (int m = 0; m < MREP; ++m)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int a = a0 + wm * WTM + m * 16 + 4 * g + reg;
        if (a >= p.Ca) continue;
        if (p.ksplit == 1 && p.bshare == 1) p.dbias[a] += accb[m][reg];
        else atomicAdd(p.dbias + a, accb[m][reg]);
      }
  }
}

// (helper of the dense tiles below)
template <int... I, class F>
__device__ __forceinline__ void rd_static_for(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}
// Fragment-read schedule of a tap wave's k-tile: T = NS x MR x NR MFMAs, m-major inside a
// substep.  Before MFMA 0: the first A row fragment and the first substep's NR B fragments
// (two reads each).  After the first MFMA of a row: the next row's A fragment.  After MFMA i of
// a substep that is not the last: the next substep's B reads i * 2 NR / M .. (i + 1) * 2 NR / M.
// LDS reads return in order, so MFMA t waits for lgkmcnt(issued - 1 - need): the reads issued
// before it, less those up to the last one it needs.
template <int MR_, int NR_>
struct RdSchedT {
  static constexpr int NS = 2, MR = MR_, NR = NR_, M = MR * NR, T = NS * M;
  static_assert(MR >= 2, "at most one B read per MFMA");
  int issued, need;
};
template <class RdSched>
constexpr RdSched rd_sched(int t_) {
  int ia[RdSched::NS * RdSched::MR] = {}, ib[RdSched::NS][RdSched::NR] = {};  // last read of each fragment
  int n = 2;
  ia[0] = n - 1;
  for (int j = 0; j < RdSched::NR; ++j) { n += 2; ib[0][j] = n - 1; }
  for (int t = 0; t < t_; ++t) {
    const int ks = t / RdSched::M, i = t % RdSched::M, m = i / RdSched::NR, j = i % RdSched::NR;
    const int gr = ks * RdSched::MR + m;
    if (j == 0 && gr + 1 < RdSched::NS * RdSched::MR) { n += 2; ia[gr + 1] = n - 1; }
    if (ks + 1 < RdSched::NS)
      for (int rr = i * 2 * RdSched::NR / RdSched::M; rr < (i + 1) * 2 * RdSched::NR / RdSched::M; ++rr)
        ib[ks + 1][rr >> 1] = n++;
  }
  const int ks = t_ / RdSched::M, i = t_ % RdSched::M;
  const int a = ia[ks * RdSched::MR + i / RdSched::NR], b = ib[ks][i % RdSched::NR];
  return RdSched{n, a > b ? a : b};
}

using RdSched = RdSchedT<5, 5>;  // (wgrad_rd_kernel's 5 x 5 blocks per tap wave)

// ---- Dense tap-per-wave tile (desc.algo 13, tile id 7): 7-wide kernels with at most 80 channels
// on each side.  The tiles above cut 75 dY channels into two 64-row tiles and 75 X channels
// into three 32-column tiles per tap (46 % of the MFMA tile space live, and three of the four
// wave rows of the second row tile idle behind the dead-block skip).  Here a block owns one
// kernel row r, all 7 taps and an 80 x 80 channel tile: 5 x 35 MFMA blocks, all live for 65..80
// channels.  Wave s (0..6) owns tap s, 5 x 5 blocks = 100 accumulator registers; the eighth
// wave has no tap: it issues its share of the DMA and sums the bias gradient (dY fragments
// against ones, as above).  Every tap wave reads the same five dY row fragments and the X halo
// shifted by its tap: 20 transposed reads per 25 MFMAs (0.8, against 1.9 on the 64 x 32 tile).
//
// LDS rows: the 160 live bytes of a pixel are kept in a 256-byte row with the 256-byte chunk
// swizzle (tr_swz); the DMA fetches only the 10 live 16-byte chunks of a row (lanes of the other
// 6 give an out-of-range offset, which moves nothing from memory and stores zeros).  Stage =
// 64 dY rows + 72 halo rows = 34 KB, ring 102 KB, one block per CU.  Bank argument: a
// transposed read takes, per 32-lane half, two 16-lane groups of 4 rows x 32 bytes (chunks
// 2c, 2c + 1 of rows R + q and R + 8 + q, q = 0..3, the same R for the whole half: R = 8 x (first
// group of the half) + K half + substep + tap).  A row is exactly one 256-byte bank row, so the
// banks of a 32-byte piece depend only on its swizzled chunk pair c ^ ((row & 3) | (bit 3 of row)
// << 2).  Rows R + q, q = 0..3, differ in row & 3; rows R + q and R + 8 + q differ in bit 3 whatever R
// is; so the 8 pieces of a half lie on 8 different chunk pairs for every tap shift: no conflict,
// for dY and for X.  A 160-byte row image would save 38 % of the ring, which nothing here needs.
//
// Pipeline, epilogue and block order are those of wgrad_rh_kernel.  18 X pieces over 8 waves:
// waves 0 and 1 issue 5 DMA instructions per k-tile, the others 4, and each waits on its own count.
constexpr int rd_lds_bytes() { return 3 * (64 + 72) * 256; }  // dynamic LDS: the ring
template <int DT>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(1)))
void wgrad_rd_kernel(const WgradRHArgs p) {
  constexpr int KP = 64, NT = 7, BM = 80, BC = 80, RB = 256;
  constexpr int MREP = BM / 16, NREP = BC / 16;
  constexpr int BYTES_A = KP * RB;
  constexpr int HROWS = 72;                  // >= 64 + NT - 1 halo pixels, whole 1 KiB pieces
  constexpr int PB = HROWS * RB / 1024;      // X pieces: 18 = 2 per wave + one more on waves 0, 1
  constexpr int STAGE = BYTES_A + HROWS * RB;
  static_assert(PB > 16 && PB <= 24 && KP * RB == 16 * 1024, "dma pieces");
  static_assert(3 * STAGE == rd_lds_bytes(), "the launcher's LDS size");

  extern __shared__ __attribute__((aligned(16))) char lds[];  // [3][STAGE]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int L = xcd_logical_block();  // = split * tiles + kernel row
  const int r0 = L % p.tiles, split = L / p.tiles;
  const int kt0 = split * p.kt_per_split;
  const int nkt = min(p.nkt, kt0 + p.kt_per_split) - kt0;
  if (nkt <= 0) return;
  // bias gradient: k-tile kt of the split is summed by the block of kernel row kt % bshare
  const bool has_bias = p.dbias != nullptr && r0 < p.bshare;
  const bool tap_wave = wave < NT;

  const int segs = p.PW / KP;
  int n = kt0 / (p.PH * segs);
  int rem = kt0 - n * p.PH * segs;
  int py = rem / segs;
  int px0 = (rem % segs) * KP;

  const __amdgpu_buffer_rsrc_t rP = dma_rsrc(p.P, p.p_bytes), rQ = dma_rsrc(p.Q, p.q_bytes);
  constexpr unsigned OOB = 0x80000000u;

  // per-lane constants of the DMA pieces (4 rows x 16 chunks each)
  //   dY piece 2 * wave + j: pixels (2 * wave + j) * 4 .. + 3 of the k-tile
  unsigned aoff[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = (wave * 2 + j) * 4 + (lane >> 4), pc = lane & 15;
    const int c = (pc ^ tr_swz<RB>(row)) << 3;
    aoff[j] = c < p.Ca ? (unsigned)((row * p.p_sw + c) * 2) : OOB;
  }
  //   X piece j * 8 + wave (< PB): halo pixels (j * 8 + wave) * 4 .. + 3
  int bhx[3], bch[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int row = (j * 8 + wave) * 4 + (lane >> 4), pc = lane & 15;
    const int c = (pc ^ tr_swz<RB>(row)) << 3;
    bhx[j] = row - p.pl;                       // + px0 = X column
    bch[j] = (c < p.Cb && row < KP + NT - 1) ? c : -1;
  }
  const bool third = wave < PB - 16;           // this wave issues a third X piece

  auto issue = [&](int slot, int n_, int py_, int px_) {
    char* st = lds + slot * STAGE;
    const int sbase = (n_ * p.p_sn + py_ * p.p_sh + px_ * p.p_sw) * 2;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const unsigned vo = aoff[j];
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rP, (__attribute__((address_space(3))) void*)(st + (wave * 2 + j) * 1024),
                                               16, vo, sbase, 0, 0);
    }
    int qy = py_ + r0 - p.pt;
    const bool yok = p.pad_mode || (unsigned)qy < (unsigned)p.QH;
    if (p.pad_mode) qy = tpg_refl(qy, p.QH);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (j == 2 && !third) break;
      int qx = px_ + bhx[j];
      bool ok = bch[j] >= 0 && yok;
      if (p.pad_mode) qx = tpg_refl(qx, p.QW);
      else ok = ok && (unsigned)qx < (unsigned)p.QW;
      const unsigned off = ok ? (unsigned)((n_ * p.q_sn + qy * p.q_sh + qx * p.q_sw + bch[j]) * 2) : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rQ, (__attribute__((address_space(3))) void*)(st + BYTES_A + (j * 8 + wave) * 1024),
                                               16, off, 0, 0, 0);
    }
  };

  // (no dead-block skip here: the tile is meant for 65..80 channels, where every block is live;
  // blocks past Ca / Cb multiply the zeros their DMA lanes stored.  The scalar branch around each
  // MFMA also kept the accumulators from staying in place: a second set of 100 registers.)
  const int g = lane >> 4, l16 = lane & 15;
  const int q = l16 >> 2, p4 = l16 & 3;
  const bool bias_wave = has_bias && !tap_wave;
  f32x4 acc[MREP][NREP], accb[MREP];
#pragma unroll
  for (int m = 0; m < MREP; ++m) {
    accb[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NREP; ++j) acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const bf16x8 ones = __builtin_bit_cast(bf16x8, u32x4{one_pair<DT>(), one_pair<DT>(), one_pair<DT>(), one_pair<DT>()});

  // per-lane LDS byte offsets of the fragment reads (as in row mode above: the substep's + 32
  // rows and, for dY, the K half's + 4 rows leave the swizzle alone and go into the offset
  // field; the tap shift does not, so the X bases carry it)
  const int tap = tap_wave ? wave : 0;
  // (absolute LDS addresses of ring slot 0; moved from slot to slot in place below, so the
  // k-tile loop holds MREP + 2 * NREP address registers and no per-slot copies of them)
  unsigned abase[MREP], bbase[NREP][2];
  const unsigned lds0 = lds_addr(lds);
#pragma unroll
  for (int m = 0; m < MREP; ++m) {
    const int col = m * 16 + 4 * p4, row = 8 * g + q;
    abase[m] = lds0 + row * RB + (((col >> 3) ^ tr_swz<RB>(row)) << 4) + (col & 7) * 2;
  }
#pragma unroll
  for (int j = 0; j < NREP; ++j)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int col = j * 16 + 4 * p4;
      const int row = 8 * g + 4 * h + q + tap;  // halo row = pixel + tap
      bbase[j][h] = lds0 + BYTES_A + row * RB + (((col >> 3) ^ tr_swz<RB>(row)) << 4) + (col & 7) * 2;
    }
  auto pin_bases = [&]() {
#pragma unroll
    for (int m = 0; m < MREP; ++m) asm volatile("" : "+v"(abase[m]));
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
      asm volatile("" : "+v"(bbase[j][0]));
      asm volatile("" : "+v"(bbase[j][1]));
    }
  };
  pin_bases();

  constexpr int NS = KP / 32;
  static_assert(NS == RdSched::NS && MREP == RdSched::MR && NREP == RdSched::NR, "fragment read schedule");
  // a tap wave's k-tile: NS x MREP x NREP MFMAs, m-major, every one behind a counted wait for its
  // own two fragments (rd_sched).  A row fragments roll through two buffers, the B fragments
  // of the next substep land in a second set while this one is used: 48 fragment registers
  // (both substeps' fragments held whole, as wgrad_rh_kernel does, are 80 and spilled).
  auto compute = [&]() {
    s16x4 fa[2][2], fb[2][NREP][2];
    auto rd_a = [&](auto grc) {  // dY fragment of global row gr = ks * MREP + m
      constexpr int gr = decltype(grc)::value, ks = gr / MREP, m = gr % MREP;
      fa[gr & 1][0] = tr_read(abase[m], (32 * ks) * RB);
      fa[gr & 1][1] = tr_read(abase[m], (32 * ks + 4) * RB);
    };
    auto rd_b = [&](auto ksc, auto rrc) {  // read rr of substep ks: half rr & 1 of X fragment rr >> 1
      constexpr int ks = decltype(ksc)::value, rr = decltype(rrc)::value;
      fb[ks & 1][rr >> 1][rr & 1] = tr_read(bbase[rr >> 1][rr & 1], 32 * ks * RB);
    };
    rd_a(std::integral_constant<int, 0>{});
    rd_static_for(std::make_integer_sequence<int, 2 * NREP>{},
                  [&](auto rrc) { rd_b(std::integral_constant<int, 0>{}, rrc); });
    __builtin_amdgcn_sched_barrier(0);
    rd_static_for(std::make_integer_sequence<int, RdSched::T>{}, [&](auto tc) {
      constexpr int t = decltype(tc)::value, ks = t / RdSched::M, i = t % RdSched::M, m = i / NREP, j = i % NREP;
      constexpr int gr = ks * MREP + m;
      constexpr RdSched sc = rd_sched<RdSched>(t);
      constexpr int w = sc.issued - 1 - sc.need < 15 ? sc.issued - 1 - sc.need : 15;
      static_assert(w >= 0, "a fragment is read before its MFMA");
      asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(w) : "memory");
      __builtin_amdgcn_sched_barrier(0);
      const bf16x8 av = __builtin_bit_cast(bf16x8, __builtin_shufflevector(fa[gr & 1][0], fa[gr & 1][1],
                                                                           0, 1, 2, 3, 4, 5, 6, 7));
      const bf16x8 bv = __builtin_bit_cast(bf16x8, __builtin_shufflevector(fb[ks & 1][j][0], fb[ks & 1][j][1],
                                                                           0, 1, 2, 3, 4, 5, 6, 7));
      acc[m][j] = mfma16x16x32<DT>(av, bv, acc[m][j]);
      // (the order rd_sched counts in: the next A row, then the next substep's B reads)
      if constexpr (j == 0 && gr + 1 < NS * MREP) rd_a(std::integral_constant<int, gr + 1>{});
      if constexpr (ks + 1 < NS) {
        constexpr int lo = i * 2 * NREP / RdSched::M, hi = (i + 1) * 2 * NREP / RdSched::M;
        if constexpr (hi > lo) rd_b(std::integral_constant<int, ks + 1>{}, std::integral_constant<int, lo>{});
        static_assert(hi - lo <= 1, "at most one B read per MFMA");
      }
      __builtin_amdgcn_sched_barrier(0);
    });
  };
  // the eighth wave's k-tile when the block owns its bias sum: the dY fragments against ones
  auto bias_sum = [&]() {
    s16x4 h[NS][2 * MREP];
#pragma unroll
    for (int ks = 0; ks < NS; ++ks)
#pragma unroll
      for (int rr = 0; rr < 2 * MREP; ++rr) h[ks][rr] = tr_read(abase[rr >> 1], (32 * ks + 4 * (rr & 1)) * RB);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < NS; ++ks)
#pragma unroll
      for (int m = 0; m < MREP; ++m)
        accb[m] = mfma16x16x32<DT>(__builtin_bit_cast(bf16x8, __builtin_shufflevector(h[ks][2 * m], h[ks][2 * m + 1],
                                                                                     0, 1, 2, 3, 4, 5, 6, 7)),
                                   ones, accb[m]);
  };

  // pipeline: k-tile i in ring slot i % 3, issued two k-tiles ahead (clamped: static vmcnt)
  int in_ = n, iy = py, ix = px0, issued = 0;  // position of the next k-tile to issue
  auto issue_next = [&](int slot) {
    issue(slot, in_, iy, ix);
    if (++issued < nkt) {
      ix += KP;
      if (ix == p.PW) { ix = 0; if (++iy == p.PH) { iy = 0; ++in_; } }
    }
  };
  // (the newest k-tile's DMAs stay in flight: 5 on waves 0 and 1, 4 on the others)
  auto wait_barrier = [&]() {
    if (third) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  };
  issue_next(0);
  issue_next(1);
  wait_barrier();  // retires k-tile 0
  // (one loop for the tap waves and one for the eighth: with both roles in one loop body the
  // accumulators did not stay in place over the MFMAs)
  auto k_loop = [&](auto tapc) {
    int slot = 0;
    for (int kt = 0; kt < nkt; ++kt) {
      issue_next(slot == 0 ? 2 : slot - 1);
      if constexpr (decltype(tapc)::value) compute();
      else if (bias_wave && (kt0 + kt) % p.bshare == r0) bias_sum();
      wait_barrier();  // retires k-tile kt+1, kt+2 stays in flight
      // the fragment bases follow the ring
      const int step = slot == 2 ? -2 * STAGE : STAGE;
#pragma unroll
      for (int m = 0; m < MREP; ++m) abase[m] += step;
#pragma unroll
      for (int j = 0; j < NREP; ++j) { bbase[j][0] += step; bbase[j][1] += step; }
      pin_bases();
      slot = slot == 2 ? 0 : slot + 1;
    }
  };
  if (tap_wave) k_loop(std::true_type{});
  else k_loop(std::false_type{});
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- epilogue as above, in chunks of 16 dW rows (one MFMA block row of every tap wave)
  constexpr int BN = NT * BC, LDC = BN + 4;
  static_assert(16 * LDC * 4 <= 3 * STAGE, "a block row of the C tile fits in the LDS ring");
  float* Cs = reinterpret_cast<float*>(lds);
  const int amax = min(BM, p.Ca);
  auto col_off = [&](int col) -> int {  // dW element offset of tile column col at a = 0; -1: padding
    const int s = col / BC, b = col % BC;
    if (b >= p.Cb) return -1;
    return b * p.w_sb + r0 * p.w_sr + s * p.w_ss;
  };
  constexpr int CG = (BN + 63) / 64;
  int coff[CG];
#pragma unroll
  for (int c = 0; c < CG; ++c) coff[c] = (c * 64 + lane < BN) ? col_off(c * 64 + lane) : -1;
  const bool vec_base = p.w_sb == 1 && (p.w_sa & 3) == 0 && ((uintptr_t)p.dW & 15) == 0;
  asm volatile("s_barrier" ::: "memory");  // (every wave's DMAs retired above: the ring is free)
#pragma unroll
  for (int m = 0; m < MREP; ++m) {
    if (m > 0) __syncthreads();  // the previous chunk has been read
    if (tap_wave) {
#pragma unroll
      for (int j = 0; j < NREP; ++j)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) Cs[(4 * g + reg) * LDC + wave * BC + j * 16 + l16] = acc[m][j][reg];
    }
    __syncthreads();
    const int rows = min(16, amax - m * 16);
    if (p.ksplit == 1) {
      constexpr int CPR = BN / 4;
      for (int idx = tid; idx < rows * CPR; idx += 512) {
        const int row = idx / CPR, cc = 4 * (idx - row * CPR);
        const float4 v = *reinterpret_cast<const float4*>(Cs + row * LDC + cc);
        float* dst = p.dW + (m * 16 + row) * p.w_sa;
        const int o0 = col_off(cc);
        if (vec_base && o0 >= 0 && (o0 & 3) == 0 && col_off(cc + 3) == o0 + 3) {
          float4* d4 = reinterpret_cast<float4*>(dst + o0);
          float4 o = *d4;
          o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
          *d4 = o;
        } else {
          const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int oe = col_off(cc + e);
            if (oe >= 0) dst[oe] += vv[e];
          }
        }
      }
    } else {
      for (int row = wave; row < rows; row += 8) {
        float* dst = p.dW + (m * 16 + row) * p.w_sa;
#pragma unroll
        for (int c = 0; c < CG; ++c)
          if (coff[c] >= 0) atomicAdd(dst + coff[c], Cs[row * LDC + c * 64 + lane]);
      }
    }
  }
  if (bias_wave && l16 == 0) {  // every column of accb holds the row sum
#pragma unroll
    for (int m = 0; m < MREP; ++m)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int a = m * 16 + 4 * g + reg;
        if (a >= p.Ca) continue;
        if (p.ksplit == 1 && p.bshare == 1) p.dbias[a] += accb[m][reg];
        else atomicAdd(p.dbias + a, accb[m][reg]);
      }
  }
}

// ---- Dense tile of NT taps (NT = 5: desc.algo 14, tile id 8, 5-wide kernels of any channel count).
// The row-halo tiles above give a wave 32 x 80 of a 128 x (5 x 32) tile: 1.87 transposed reads per
// MFMA, and 80 channels pad to 128 x 96.  Here a block owns one kernel row r, all NT taps, an a-tile
// of p.tm dY channels and a b-tile of p.tn X channels (the planner cuts C channels into
// ceil(C / 112) tiles of ceil(C / tiles) rounded up to 16: 206 -> 112 + 94, 80 -> 80, 64 -> 64), so
// NT x NB column blocks (tap, b-block), NB = p.tn / 16.  They are dealt to the 8 waves in fixed
// order: slot j of wave w is column block w + 8 j = tap * NB + b-block, and every wave holds all
// MR block rows of its NRW = ceil(NT NB / 8) slots.  Every wave reads the same MR dY row fragments
// and its own X fragments at (tap shift, b-block) offsets, which are per-wave uniform and live in
// the per-lane base addresses: (2 MR + 2 NRW) reads per MR x NRW MFMAs, 24 / 35 on the 112 x 112
// tile.  Block rows past p.tm and slots past NT NB multiply zeros (no branch around an MFMA):
// the rows were stored as zeros by the DMA, the slots read a zero constant behind the ring.
// 8 NRW > NT NB for every tile the launcher gives an instance, so the last slot of wave 7 is always
// spare: it reads a constant of ones during the k-tiles whose bias sum the block owns (zeros
// otherwise) and its accumulators are the dY row sums.  (<NT = 7, MR = 5, NRW = 5> is algo 13 bit
// for bit and lost the launch timing to wgrad_rd_kernel, profiles/r14/refactor_ab.txt: not built.)
//
// LDS rows, DMA, ring, pipeline, read schedule, block order and epilogue are wgrad_rd_kernel's
// (a 256-byte row holds up to 128 channels of a tile; only the live chunks are fetched).

// dynamic LDS: the ring, then the constants (1 KiB of ones and zeros, and again SUB further on)
constexpr int dense_lds_bytes() { return rd_lds_bytes() + 32 * 256 + 1024; }

template <int DT, int NT, int MR, int NRW>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(1)))
void wgrad_dense_kernel(const WgradRHArgs p) {
  constexpr int KP = 64, RB = 256;
  constexpr int BYTES_A = KP * RB;
  constexpr int HROWS = 72;                  // >= 64 + NT - 1 halo pixels, whole 1 KiB pieces
  constexpr int PB = HROWS * RB / 1024;      // X pieces: 18 = 2 per wave + one more on waves 0, 1
  constexpr int STAGE = BYTES_A + HROWS * RB;
  constexpr int SUB = 32 * RB;               // LDS bytes from a substep's rows to the next one's
  // constants behind the ring: 512 bytes of ones, then 512 of zeros, and again SUB further on
  // (a spare slot's lanes read 8 bytes each at lane * 8, plus the substep's offset field)
  constexpr int CONSTS = 3 * STAGE;
  using Sched = RdSchedT<MR, NRW>;
  static_assert(PB > 16 && PB <= 24 && KP * RB == 16 * 1024 && KP + NT - 1 <= HROWS, "dma pieces");
  static_assert(CONSTS + SUB + 1024 == dense_lds_bytes(), "the launcher's LDS size");
  static_assert(MR <= 7 && NRW <= 5, "tiles of at most 112 x 112 channels");

  extern __shared__ __attribute__((aligned(16))) char lds[];  // [3][STAGE], constants
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int L = xcd_logical_block();  // = split * tiles + (a-tile, b-tile, kernel row)
  const int tile = L % p.tiles, split = L / p.tiles;
  const int ta = tile % p.nta, tb = (tile / p.nta) % p.ntb, r0 = tile / (p.nta * p.ntb);
  const int a0 = ta * p.tm, b0 = tb * p.tn;
  const int alim = min(p.Ca, a0 + p.tm), blim = min(p.Cb, b0 + p.tn);
  const int NB = p.tn >> 4, ncb = NT * NB;   // column blocks of the tile
  const int kt0 = split * p.kt_per_split;
  const int nkt = min(p.nkt, kt0 + p.kt_per_split) - kt0;
  if (nkt <= 0) return;
  // bias gradient: k-tile kt of the split is summed by the a-tile's block (b-tile, kernel row)
  // of share index kt % bshare
  const int sid = tb + p.ntb * r0;
  const bool bias_wave = p.dbias != nullptr && sid < p.bshare && wave == 7;

  const int segs = p.PW / KP;
  int n = kt0 / (p.PH * segs);
  int rem = kt0 - n * p.PH * segs;
  int py = rem / segs;
  int px0 = (rem % segs) * KP;

  const __amdgpu_buffer_rsrc_t rP = dma_rsrc(p.P, p.p_bytes), rQ = dma_rsrc(p.Q, p.q_bytes);
  constexpr unsigned OOB = 0x80000000u;

  // per-lane constants of the DMA pieces (4 rows x 16 chunks each; chunk pc of a row holds the
  // tile's channels 8 * (pc ^ swizzle) ..)
  //   dY piece 2 * wave + j: pixels (2 * wave + j) * 4 .. + 3 of the k-tile
  unsigned aoff[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = (wave * 2 + j) * 4 + (lane >> 4), pc = lane & 15;
    const int c = a0 + ((pc ^ tr_swz<RB>(row)) << 3);
    aoff[j] = c < alim ? (unsigned)((row * p.p_sw + c) * 2) : OOB;
  }
  //   X piece j * 8 + wave (< PB): halo pixels (j * 8 + wave) * 4 .. + 3
  int bhx[3], bch[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int row = (j * 8 + wave) * 4 + (lane >> 4), pc = lane & 15;
    const int c = b0 + ((pc ^ tr_swz<RB>(row)) << 3);
    bhx[j] = row - p.pl;                       // + px0 = X column
    bch[j] = (c < blim && row < KP + NT - 1) ? c : -1;
  }
  const bool third = wave < PB - 16;           // this wave issues a third X piece

  auto issue = [&](int slot, int n_, int py_, int px_) {
    char* st = lds + slot * STAGE;
    const int sbase = (n_ * p.p_sn + py_ * p.p_sh + px_ * p.p_sw) * 2;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const unsigned vo = aoff[j];
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rP, (__attribute__((address_space(3))) void*)(st + (wave * 2 + j) * 1024),
                                               16, vo, sbase, 0, 0);
    }
    int qy = py_ + r0 - p.pt;
    const bool yok = p.pad_mode || (unsigned)qy < (unsigned)p.QH;
    if (p.pad_mode) qy = tpg_refl(qy, p.QH);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (j == 2 && !third) break;
      int qx = px_ + bhx[j];
      bool ok = bch[j] >= 0 && yok;
      if (p.pad_mode) qx = tpg_refl(qx, p.QW);
      else ok = ok && (unsigned)qx < (unsigned)p.QW;
      const unsigned off = ok ? (unsigned)((n_ * p.q_sn + qy * p.q_sh + qx * p.q_sw + bch[j]) * 2) : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rQ, (__attribute__((address_space(3))) void*)(st + BYTES_A + (j * 8 + wave) * 1024),
                                               16, off, 0, 0, 0);
    }
  };

  const int g = lane >> 4, l16 = lane & 15;
  const int q = l16 >> 2, p4 = l16 & 3;
  f32x4 acc[MR][NRW];
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int j = 0; j < NRW; ++j) acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the constants (made visible by the first k-tile's barrier)
  if (tid < 256) {
    const unsigned v = tid < 128 ? one_pair<DT>() : 0u;
    unsigned* cs = reinterpret_cast<unsigned*>(lds + CONSTS);
    cs[tid] = v;
    cs[tid + SUB / 4] = v;
  }

  // per-lane LDS byte addresses of the fragment reads in ring slot 0 (as in wgrad_rd_kernel: the
  // substep's + 32 rows and, for dY, the K half's + 4 rows go into the offset field; the X bases
  // carry the slot's tap shift and b-block).  Spare slots stay on the constants.
  unsigned abase[MR], bbase[NRW][2];
  const unsigned lds0 = lds_addr(lds);
  const unsigned zeros = lds0 + CONSTS + 512 + lane * 8;
  // the last slot of a wave when it is spare: ones while the block's bias wave owns k-tile kt
  auto spare_base = [&](int kt) -> unsigned {
    return bias_wave && (kt0 + kt) % p.bshare == sid ? zeros - 512 : zeros;
  };
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    const int col = m * 16 + 4 * p4, row = 8 * g + q;
    abase[m] = lds0 + row * RB + (((col >> 3) ^ tr_swz<RB>(row)) << 4) + (col & 7) * 2;
  }
  bool slot_live[NRW];
#pragma unroll
  for (int j = 0; j < NRW; ++j) {
    const int cb = wave + 8 * j;
    slot_live[j] = cb < ncb;
    const int tap = slot_live[j] ? cb / NB : 0, bb = slot_live[j] ? cb % NB : 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int col = bb * 16 + 4 * p4;
      const int row = 8 * g + 4 * h + q + tap;  // halo row = pixel + tap
      const unsigned live = lds0 + BYTES_A + row * RB + (((col >> 3) ^ tr_swz<RB>(row)) << 4) + (col & 7) * 2;
      bbase[j][h] = slot_live[j] ? live : (j == NRW - 1 ? spare_base(0) : zeros);
    }
  }
  auto pin_bases = [&]() {
#pragma unroll
    for (int m = 0; m < MR; ++m) asm volatile("" : "+v"(abase[m]));
#pragma unroll
    for (int j = 0; j < NRW; ++j) {
      asm volatile("" : "+v"(bbase[j][0]));
      asm volatile("" : "+v"(bbase[j][1]));
    }
  };
  pin_bases();

  // a wave's k-tile: NS x MR x NRW MFMAs, m-major, every one behind a counted wait for its own two
  // fragments (rd_sched); rolling A and double-set B fragment registers as in wgrad_rd_kernel
  constexpr int NS = Sched::NS;
  static_assert(NS * 32 == KP, "substeps");
  auto compute = [&]() {
    s16x4 fa[2][2], fb[2][NRW][2];
    auto rd_a = [&](auto grc) {  // dY fragment of global row gr = ks * MR + m
      constexpr int gr = decltype(grc)::value, ks = gr / MR, m = gr % MR;
      fa[gr & 1][0] = tr_read(abase[m], ks * SUB);
      fa[gr & 1][1] = tr_read(abase[m], ks * SUB + 4 * RB);
    };
    auto rd_b = [&](auto ksc, auto rrc) {  // read rr of substep ks: half rr & 1 of X fragment rr >> 1
      constexpr int ks = decltype(ksc)::value, rr = decltype(rrc)::value;
      fb[ks & 1][rr >> 1][rr & 1] = tr_read(bbase[rr >> 1][rr & 1], ks * SUB);
    };
    rd_a(std::integral_constant<int, 0>{});
    rd_static_for(std::make_integer_sequence<int, 2 * NRW>{},
                  [&](auto rrc) { rd_b(std::integral_constant<int, 0>{}, rrc); });
    __builtin_amdgcn_sched_barrier(0);
    rd_static_for(std::make_integer_sequence<int, Sched::T>{}, [&](auto tc) {
      constexpr int t = decltype(tc)::value, ks = t / Sched::M, i = t % Sched::M, m = i / NRW, j = i % NRW;
      constexpr int gr = ks * MR + m;
      constexpr Sched sc = rd_sched<Sched>(t);
      constexpr int w = sc.issued - 1 - sc.need < 15 ? sc.issued - 1 - sc.need : 15;
      static_assert(w >= 0, "a fragment is read before its MFMA");
      asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(w) : "memory");
      __builtin_amdgcn_sched_barrier(0);
      const bf16x8 av = __builtin_bit_cast(bf16x8, __builtin_shufflevector(fa[gr & 1][0], fa[gr & 1][1],
                                                                           0, 1, 2, 3, 4, 5, 6, 7));
      const bf16x8 bv = __builtin_bit_cast(bf16x8, __builtin_shufflevector(fb[ks & 1][j][0], fb[ks & 1][j][1],
                                                                           0, 1, 2, 3, 4, 5, 6, 7));
      acc[m][j] = mfma16x16x32<DT>(av, bv, acc[m][j]);
      // (the order rd_sched counts in: the next A row, then the next substep's B reads)
      if constexpr (j == 0 && gr + 1 < NS * MR) rd_a(std::integral_constant<int, gr + 1>{});
      if constexpr (ks + 1 < NS) {
        constexpr int lo = i * 2 * NRW / Sched::M, hi = (i + 1) * 2 * NRW / Sched::M;
        if constexpr (hi > lo) rd_b(std::integral_constant<int, ks + 1>{}, std::integral_constant<int, lo>{});
        static_assert(hi - lo <= 1, "at most one B read per MFMA");
      }
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  // pipeline: k-tile i in ring slot i % 3, issued two k-tiles ahead (clamped: static vmcnt)
  int in_ = n, iy = py, ix = px0, issued = 0;  // position of the next k-tile to issue
  auto issue_next = [&](int slot) {
    issue(slot, in_, iy, ix);
    if (++issued < nkt) {
      ix += KP;
      if (ix == p.PW) { ix = 0; if (++iy == p.PH) { iy = 0; ++in_; } }
    }
  };
  // (the newest k-tile's DMAs stay in flight: 5 on waves 0 and 1, 4 on the others)
  auto wait_barrier = [&]() {
    if (third) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  };
  issue_next(0);
  issue_next(1);
  wait_barrier();  // retires k-tile 0 (and the constants)
  int slot = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    issue_next(slot == 0 ? 2 : slot - 1);
    compute();
    wait_barrier();  // retires k-tile kt+1, kt+2 stays in flight
    // the fragment bases follow the ring; the spare slots stay, the last one by the bias share
    const int step = slot == 2 ? -2 * STAGE : STAGE;
#pragma unroll
    for (int m = 0; m < MR; ++m) abase[m] += step;
#pragma unroll
    for (int j = 0; j < NRW; ++j) {
      const int sj = slot_live[j] ? step : 0;
      bbase[j][0] += sj;
      bbase[j][1] += sj;
    }
    if (!slot_live[NRW - 1]) bbase[NRW - 1][0] = bbase[NRW - 1][1] = spare_base(kt + 1);
    pin_bases();
    slot = slot == 2 ? 0 : slot + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- epilogue as above, in chunks of 16 dW rows (one MFMA block row of every wave); tile
  // column = column block * 16 + l16 = tap * p.tn + b
  const int BN = ncb * 16, LDC = BN + 4;
  static_assert(16 * (NT * 112 + 4) * 4 <= 3 * STAGE, "a block row of the C tile fits in the LDS ring");
  float* Cs = reinterpret_cast<float*>(lds);
  const int amax = alim - a0;
  auto col_off = [&](int col) -> int {  // dW element offset of tile column col at a = 0; -1: padding
    const int s = col / p.tn, b = b0 + col % p.tn;
    if (b >= p.Cb) return -1;
    return b * p.w_sb + r0 * p.w_sr + s * p.w_ss;
  };
  constexpr int CG = 2 * NRW;  // 64-column groups: NT NB <= 8 NRW
  int coff[CG];
#pragma unroll
  for (int c = 0; c < CG; ++c) coff[c] = (c * 64 + lane < BN) ? col_off(c * 64 + lane) : -1;
  const bool vec_base = p.w_sb == 1 && (p.w_sa & 3) == 0 && ((uintptr_t)p.dW & 15) == 0;
  asm volatile("s_barrier" ::: "memory");  // (every wave's DMAs retired above: the ring is free)
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    if (m > 0) __syncthreads();  // the previous chunk has been read
#pragma unroll
    for (int j = 0; j < NRW; ++j)
      if (slot_live[j]) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) Cs[(4 * g + reg) * LDC + (wave + 8 * j) * 16 + l16] = acc[m][j][reg];
      }
    __syncthreads();
    const int rows = min(16, amax - m * 16);  // (<= 0 past the a-tile: nothing to add)
    if (p.ksplit == 1) {
      const int CPR = BN / 4;
      for (int idx = tid; idx < rows * CPR; idx += 512) {
        const int row = idx / CPR, cc = 4 * (idx - row * CPR);
        const float4 v = *reinterpret_cast<const float4*>(Cs + row * LDC + cc);
        float* dst = p.dW + (a0 + m * 16 + row) * p.w_sa;
        const int o0 = col_off(cc);
        if (vec_base && o0 >= 0 && (o0 & 3) == 0 && col_off(cc + 3) == o0 + 3) {
          float4* d4 = reinterpret_cast<float4*>(dst + o0);
          float4 o = *d4;
          o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
          *d4 = o;
        } else {
          const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int oe = col_off(cc + e);
            if (oe >= 0) dst[oe] += vv[e];
          }
        }
      }
    } else {
      for (int row = wave; row < rows; row += 8) {
        float* dst = p.dW + (a0 + m * 16 + row) * p.w_sa;
#pragma unroll
        for (int c = 0; c < CG; ++c)
          if (coff[c] >= 0) atomicAdd(dst + coff[c], Cs[row * LDC + c * 64 + lane]);
      }
    }
  }
  if (bias_wave && l16 == 0) {  // every column of the spare slot holds the row sum
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int a = a0 + m * 16 + 4 * g + reg;
        if (a >= alim) continue;
        if (p.ksplit == 1 && p.bshare == 1) p.dbias[a] += acc[m][NRW - 1][reg];
        else atomicAdd(p.dbias + a, acc[m][NRW - 1][reg]);
      }
  }
}

// tile configs {id, BM, BC}; id = desc.algo - 6 (ids 4, 5: image mode, 32-channel b tiles;
// id 6: row mode, 256 dY channels per block, waves 64 x (NT x 32) / 2; id 7: the dense
// 80 x (7 x 80) tile, wgrad_rd_kernel; id 8: the dense five-tap tile, wgrad_dense_kernel -- its
// largest; the planner fits them to the channels)
#define TPG_WGRAD_RH_CFGS(X) \
  X(0, 128, 64)              \
  X(1, 128, 32)              \
  X(2, 64, 64)               \
  X(3, 64, 32)               \
  X(4, 128, 32)              \
  X(5, 64, 32)               \
  X(6, 256, 32)              \
  X(7, 80, 80)               \
  X(8, 112, 112)

int wgrad_rh_tile(int cfg, int* bm, int* bc) {
#define X(id, BM_, BC_) if (cfg == (id)) { *bm = BM_; *bc = BC_; return 0; }
  TPG_WGRAD_RH_CFGS(X)
#undef X
  return -1;
}

// sets the dynamic-LDS limit of a kernel's bf16 / fp16 pair once and launches one of the two:
// tiles * ksplit blocks of 512 threads
template <auto K1, auto K2, int LDS>
static int launch_pair(const WgradRHArgs& a, hipStream_t s) {
  static bool once = ((void)hipFuncSetAttribute((const void*)K1, hipFuncAttributeMaxDynamicSharedMemorySize, LDS),
                      (void)hipFuncSetAttribute((const void*)K2, hipFuncAttributeMaxDynamicSharedMemorySize, LDS),
                      true);
  (void)once;
  hipLaunchKernelGGL(a.dtype == 2 ? K2 : K1, dim3(a.tiles * a.ksplit), dim3(512), LDS, s, a);
  return (int)hipGetLastError();
}

template <int NT, int MR, int NRW>
static int launch_dense_t(const WgradRHArgs& a, hipStream_t s) {
  return launch_pair<wgrad_dense_kernel<1, NT, MR, NRW>, wgrad_dense_kernel<2, NT, MR, NRW>, dense_lds_bytes()>(a, s);
}

// five-tap tiles: the smallest instance (block rows, column slots per wave) that holds the tile:
// 112 x 112 (7, 5), 80 x 80 (5, 4), 64 x 112 (4, 5).  (A (4, 3) instance for 64 x 64 was correct and
// lost its sweep to the 64 x 32 row-halo tile on the 64 -> 64 layer, so it is not built: such tiles
// run on (4, 5).)
static int launch_dense5(const WgradRHArgs& a, hipStream_t s) {
  constexpr int NT = 5;
  // (nb <= 7, and nb <= 6 where nrw <= 4: wave 7's last slot, column block 8 NRW - 1, stays spare)
  static_assert(8 * 5 > NT * 7 && 8 * 4 > NT * 6, "the bias slot");
  const int mr = a.tm / 16, nb = a.tn / 16, nrw = (NT * nb + 7) / 8;
  if (mr <= 4) return launch_dense_t<NT, 4, 5>(a, s);
  if (mr <= 5 && nrw <= 4) return launch_dense_t<NT, 5, 4>(a, s);
  return launch_dense_t<NT, 7, 5>(a, s);
}

static int launch_rd(const WgradRHArgs& a, hipStream_t s) {
  return launch_pair<wgrad_rd_kernel<1>, wgrad_rd_kernel<2>, rd_lds_bytes()>(a, s);
}

template <int NR, int NT, int BM, int BC>
static int launch_rh_t(const WgradRHArgs& a, hipStream_t s) {
  return launch_pair<wgrad_rh_kernel<1, NR, NT, BM, BC>, wgrad_rh_kernel<2, NR, NT, BM, BC>, rh_lds_bytes<NR, BM, BC>()>(a, s);
}

// row-mode configs instantiate the 1 x {3,4,5} tap groups, image-mode ones the 2x2 / 3x3 (the
// dense ids 7 and 8 have their own launchers)
template <int ID, int BM, int BC>
static int launch_rh_cfg(const WgradRHArgs& a, hipStream_t s) {
  if constexpr (ID < 4 || ID == 6) {
    if (a.nr == 1 && a.nt == 3) return launch_rh_t<1, 3, BM, BC>(a, s);
    if (a.nr == 1 && a.nt == 4) return launch_rh_t<1, 4, BM, BC>(a, s);
    if (a.nr == 1 && a.nt == 5) return launch_rh_t<1, 5, BM, BC>(a, s);
    // a whole 7-tap kernel row per block (7x7 convs): the 4 + 4 grouping computed a dead tap
    // column; only the tiles whose 7 x BC columns keep the fragments within the VGPR budget
    if constexpr (ID >= 1 && ID <= 3)
      if (a.nr == 1 && a.nt == 7) return launch_rh_t<1, 7, BM, BC>(a, s);
  } else if constexpr (ID < 6) {
    if (a.nr == 2 && a.nt == 2) return launch_rh_t<2, 2, BM, BC>(a, s);
    if (a.nr == 3 && a.nt == 3) return launch_rh_t<3, 3, BM, BC>(a, s);
  }
  return -1;
}

int launch_wgrad_rh(const WgradRHArgs& a, hipStream_t s) {
  if (a.cfg == 7 && a.nr == 1 && a.nt == 7 && a.kw == 7 && a.Ca <= 80 && a.Cb <= 80 && a.tw == 64 && a.tiles == a.kh)
    return launch_rd(a, s);
  if (a.cfg == 8 && a.nr == 1 && a.nt == 5 && a.kw == 5 && a.tw == 64 && a.tm >= 16 && a.tm <= 112 && a.tm % 16 == 0 &&
      a.tn >= 16 && a.tn <= 112 && a.tn % 16 == 0 && a.nta * a.tm >= a.Ca && a.ntb * a.tn >= a.Cb &&
      a.tiles == a.nta * a.ntb * a.kh)
    return launch_dense5(a, s);
#define X(id, BM_, BC_) \
  if (a.cfg == (id)) return launch_rh_cfg<id, BM_, BC_>(a, s);
  TPG_WGRAD_RH_CFGS(X)
#undef X
  return -1;
}

}  // namespace tpg
