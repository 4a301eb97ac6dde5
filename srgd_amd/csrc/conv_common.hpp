// Building blocks the convolution kernels share (conv3x3_bf16 / _mxfp8 / _mx2 / _split, conv1x1_bf16 / _mxfp8 / _split, conv_igemm; the
// synchronisation vocabulary also serves linattn_fused*.hip): counted waits and the raw barrier, the LDS row swizzle and LDS-DMA, the
// XCD band remap and the 3x3 patch-tile decode, the (hi, lo) operand split with the GroupNorm-in-staging transform, and the slot layout and
// slot counter of the GroupNorm partial sums.  common.hpp stays the general helper file.  What a kernel schedules - K loops, wait counts,
// barrier placement, LDS layouts, launchers - stays in its own file; what lives here is ONE copy of what those files used to paste.
#pragma once
#include "kernels.hpp"

namespace srgd {

typedef __attribute__((address_space(3))) void* lds_ptr;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));

// ---- synchronisation and LDS vocabulary ---------------------------------------------------------------------------------------------
// Counted wait: LDS-DMA prefetches stay in flight across barriers; vmcnt retires a wave's vector-memory requests in issue order.
#define WAIT_VM(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")
// Raw barrier (no vmcnt drain: LDS-DMA prefetches stay in flight) fenced for the instruction scheduler:
// s_barrier is IntrNoMem to LLVM, so without sched_barrier(0) the machine scheduler hoists the next step's
// ds_reads above it - a read of a buffer whose DMA other waves have not yet waited for.
#define BARRIER()                        \
  do {                                   \
    __builtin_amdgcn_s_barrier();        \
    __builtin_amdgcn_sched_barrier(0);   \
  } while (0)

// Row swizzle of the 64-byte LDS rows: chunk ^= (row >> 1) & 3 for the 16x16x32 operand pattern (16 rows x 4 chunks per ds_read_b128) -
// conflict-free for its lane groups at every tap shift (checked exhaustively on the bank model).
__device__ __forceinline__ int row_swz(int row) { return (row >> 1) & 3; }

// LDS-DMA, 16 bytes per lane, no VGPR round trip: LDS destination = wave-uniform base + lane * 16; voffset per lane (VGPR), soffset
// wave-uniform (SGPR) - keeping the uniform part out of the VGPRs
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, char* lds_wave_base, int voffset, int soffset = 0) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr)lds_wave_base, 16, voffset, soffset, 0, 0);
}

// ---- tile maps ----------------------------------------------------------------------------------------------------------------------
// XCD-aware remap of a workgroup id: the hardware deals consecutive ids round-robin to the 8 XCDs (one private L2 each), so ids b,
// b + 8, ... share an XCD; the remap gives each XCD a contiguous band of logical tiles (halo and weight reuse in its L2).
// Tile map, measured with the L2's own counters (round 5, profiles/r5/conv3x3_bf16_tcc_*.txt; 1024 -> 1024 @32^2, 125 tiles):
// this map - n-tiles fastest inside an XCD's band, so the 64 workgroups an XCD runs at a time are 8 m-tiles x 8 n-tiles - reads
// 112.7 M 128-byte lines per launch with an 81 % L2 hit rate (23.4 M misses = 3.0 GB from the Infinity Cache).  Pinning one
// n-tile per XCD makes the weight stream L2-resident and every XCD read every halo patch: 21.4 M misses, the same clock and
// throughput.  Blocks of 32 m-tiles x 2 n-tiles cut the misses to 17.1 M (-27 %): clock 1.653 vs 1.648 GHz, +0.4 % (noise).
// Non-temporal halo DMAs and output stores: 29-36 M misses, 1.55-1.59 GHz, -4 ... -12 %.  The kernel's clock does not follow
// its traffic beyond L2 within what a tile map can change, so the simplest map stays.
__device__ __forceinline__ int xcd_band_remap(int wg, int nwg) {
  const int q = nwg >> 3, rem = nwg & 7, x = wg & 7, k = wg >> 3;
  return (x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q) + k;
}

// The tile of a 3x3 patch kernel (output tile = an 8 x PW pixel patch x 128 channels; grid = B * tiles_y * tiles_x * n_tiles): n-tile
// nt, sample b, patch trem inside the sample (the GroupNorm slot index is built from it) with origin (y0, x0), n-tiles fastest.
// Results through references and the arguments in this order on purpose: returned as a struct, or with (B, H, W, Cout) in the
// natural order, the kernels' tile arithmetic compiles to a different operand order (same values, not the same instructions).
template <int PW>
__device__ __forceinline__ void patch_tile_decode(int wg, int Cout, int W, int H, int B, int& n_tiles, int& tiles_x, int& tiles_y, int& nt,
                                                  int& b, int& trem, int& y0, int& x0) {
  n_tiles = Cout / 128;
  tiles_x = W / PW, tiles_y = H / 8;
  const int m_tiles = B * tiles_y * tiles_x;
  wg = xcd_band_remap(wg, m_tiles * n_tiles);
  nt = wg % n_tiles;
  const int mt = wg / n_tiles;
  b = mt / (tiles_y * tiles_x);
  trem = mt - b * tiles_y * tiles_x;
  const int ty = trem / tiles_x, tx = trem - ty * tiles_x;
  y0 = ty * 8, x0 = tx * PW;
}

// ---- the (hi, lo) operand split -----------------------------------------------------------------------------------------------------
// A note for everything below that takes values out of a packed register vector: copy the element into a local first
// (`const unsigned u = r[k];`).  __builtin_bit_cast applied directly to the vector-element lvalue r[k] read element 0 for every k
// with this toolchain - hipcc 7.2 - which the kernel tests caught.
//
// The f16 hi half of a pair: a FINITE value beyond f16's range saturates at +-65504 (finite garbage instead of inf - inf = NaN;
// activations on this path are O(1..100)); a NaN or an infinity leaves as NaN in both halves and so reaches every output it
// contributes to (sat_f16_keep_nonfinite, common.hpp).  a and b come back saturated, hf holds the hi halves as floats.
__device__ __forceinline__ unsigned split_hi_f16(float& a, float& b, f32x2& hf) {
  a = sat_f16_keep_nonfinite(a);
  b = sat_f16_keep_nonfinite(b);
  const f16x2 h = __builtin_convertvector(f32x2{a, b}, f16x2);
  hf = __builtin_convertvector(h, f32x2);
  return __builtin_bit_cast(unsigned, h);
}
// two fp32 -> their packed hi and lo 16-bit halves.  bf16 halves share fp32's range: no clamp.
template <bool F16>
__device__ __forceinline__ void split_pair(float a, float b, unsigned& hi, unsigned& lo) {
  if constexpr (F16) {
    f32x2 hf;
    hi = split_hi_f16(a, b, hf);
    const f16x2 l = __builtin_convertvector(f32x2{a - hf[0], b - hf[1]}, f16x2);
    lo = __builtin_bit_cast(unsigned, l);
  } else {
    const bf16x2 h = __builtin_convertvector(f32x2{a, b}, bf16x2);
    const unsigned hb = __builtin_bit_cast(unsigned, h);
    const float h0 = __uint_as_float(hb << 16), h1 = __uint_as_float(hb & 0xffff0000u);
    const bf16x2 l = __builtin_convertvector(f32x2{a - h0, b - h1}, bf16x2);
    hi = hb;
    lo = __builtin_bit_cast(unsigned, l);
  }
}
// 8 fp32 (two 16-byte vectors) -> 8 hi + 8 lo 16-bit values (each a 16-byte operand fragment)
template <bool F16>
__device__ __forceinline__ void split8(const u32x4& r0, const u32x4& r1, u32x4& hi, u32x4& lo) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned ua = k < 2 ? r0[2 * k] : r1[2 * k - 4], ub = k < 2 ? r0[2 * k + 1] : r1[2 * k - 3];
    unsigned h, l;
    split_pair<F16>(__uint_as_float(ua), __uint_as_float(ub), h, l);
    hi[k] = h;
    lo[k] = l;
  }
}

// GNIN: the PRODUCER's GroupNorm-apply + SiLU (reference Block.forward model.py:250-259 between two convolutions) on four packed fp32
// of a halo piece, in registers, ahead of the split.  v_exp_f32 / v_rcp_f32 (1 ulp each) instead of gn_apply's expf and IEEE
// division: ~3e-7 relative, far inside the split modes' 2^-22 per product.
__device__ __forceinline__ void act4(u32x4& r, const f32x4& ga, const f32x4& gb) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned u = r[k];                       // (copied out first: see the note above)
    const float t = __builtin_fmaf(ga[k], __uint_as_float(u), gb[k]);
    r[k] = __float_as_uint(t * __builtin_amdgcn_rcpf(1.0f + __expf(-t)));
  }
}

// ---- GroupNorm partial sums of the register-direct 3x3 epilogues ----------------------------------------------------------------------
// The tail of the 3x3 patch kernels: per-(sample, group) sums of a wave's pixels x 64 channels, in-lane over the register positions
// (s1v, s2v: the lane's sums and sums of squares), over the 16 pixels of a row by DPP, then over the rows that share a group (fixed
// order: deterministic).  cpg = channels per group:
//   16: one group per lane row (q16) -> four groups, written by lanes 0, 16, 32, 48;   32: row pairs -> lanes 0 and 32;
//   >= 64: the whole wave -> lane 0.
// Slot layout: [b][group][(patch, n-tile of the group) x contributing waves]: the WAVES_M waves (wm) of the group's column half, or
// all 2 * WAVES_M when a group spans the whole TILE_N-channel tile (WAVES_M = 4, 2 for the 256-thread kernels); gn_finalize sums the
// slots in index order (fp64) - a tail that disagrees with the counter below is a silent wrong statistic.
// chw = first channel of the wave's 64, chl = the lane row's offset in them (16 * q16); trem, nt, b, tiles_y, tiles_x: patch_tile_decode.
// Called by conv3x3_split (both forms) and conv3x3_mxfp8.  conv3x3_bf16 and conv3x3_mx2 keep a copy of this body: through the call
// their instruction streams changed (profiles/conv_common_refactor.txt).
template <int TILE_N, int WAVES_M>
__device__ __forceinline__ void gn_partial_store(const f32x4& s1v, const f32x4& s2v, int Cout, int groups, float* gn_partial, int r16, int q16,
                                                 int wave, int wm, int tiles_y, int tiles_x, int trem, int nt, int b, int chw, int chl) {
  const int cpg = Cout / groups;                        // 16, 32, 64 or a multiple of TILE_N
  float a1 = row16_sum((s1v[0] + s1v[1]) + (s1v[2] + s1v[3]));
  float a2 = row16_sum((s2v[0] + s2v[1]) + (s2v[2] + s2v[3]));
  if (cpg >= 32) { a1 = xor16_sum(a1); a2 = xor16_sum(a2); }
  if (cpg >= 64) { a1 = xor32_sum(a1); a2 = xor32_sum(a2); }
  const int rows_per_group = cpg >= 64 ? 4 : cpg >> 4;
  if (r16 == 0 && (q16 & (rows_per_group - 1)) == 0) {
    const int tpg = cpg >= TILE_N ? cpg / TILE_N : 1;   // TILE_N-channel tiles per group
    const int wpt = cpg >= TILE_N ? 2 * WAVES_M : WAVES_M;   // contributing waves per tile
    const int nslots = tiles_y * tiles_x * tpg * wpt;
    const int slot = (trem * tpg + (cpg >= TILE_N ? nt % tpg : 0)) * wpt + (cpg >= TILE_N ? wave : wm);
    const int g = cpg >= TILE_N ? chw / cpg : (chw + chl) >> __builtin_ctz(cpg);      // cpg < TILE_N: a power of two (eligibility)
    float* dst = gn_partial + ((size_t)(b * groups + g) * nslots + slot) * 2;
    *reinterpret_cast<f32x2*>(dst) = f32x2{a1, a2};
  }
}
// host: slots per (sample, group) that such a tail writes over an image of 8 x 32 pixel patches (the 256-thread
// split kernel has twice the patches with half the waves each: the same count)
static inline int conv3x3_stats_slots(const ConvArgs& a, int waves_m) {
  if (a.groups <= 0) return 0;
  const int cpg = a.Cout / a.groups;
  return (a.Hin / 8) * (a.Win / 32) * (cpg >= 128 ? (cpg / 128) * 2 * waves_m : waves_m);
}

}  // namespace srgd
