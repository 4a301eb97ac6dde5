// 3x3 / stride 1 / pad 1 convolution in SPLIT-OPERAND precision for gfx950 (MI355X): fp32 activations and fp32 results in HBM,
// the contraction on the 16-bit matrix cores with every operand carried as a (hi, lo) pair of 16-bit values,
//     x = x_hi + x_lo,   w = w_hi + w_lo,   x * w ~= x_hi * w_hi + x_lo * w_hi + x_hi * w_lo      (fp32 accumulate),
// i.e. three v_mfma_f32_16x16x32_{f16,bf16} per fragment pair.  The dropped x_lo * w_lo term and the rounding of the lo halves are
// 2^-22 (f16 halves, 11 + 11 significand bits) or 2^-16 (bf16 halves) of a product - against 2^-9 for plain bf16 operands.
// The purpose: a precision that meets the reference's 1e-3 parity bar (reference Block.proj, model.py:246,
// computes in fp32) at a third of the bf16 MFMA rate instead of the 1/16 of the exact-fp32 MFMA (conv_igemm.hip).
//
// Same implicit GEMM and the same LDS images as conv3x3_bf16.hip (M = an 8 x 32 pixel patch, N = 128 output channels, K walked
// channel-chunk-major with the (8+2) x (32+2) halo patch of a 32-channel chunk staged once for all nine taps; 64-byte LDS rows,
// XOR-swizzled; weights as srcA so that the epilogue is register-direct), with these differences:
//   * the halo patch arrives as fp32 through VGPRs (buffer_load_dwordx4, out-of-image pixels zero-filled by the descriptor's range
//     check), is split in registers (v_cvt_pk + v_sub: ~3 VALU per element, 24 elements per thread and chunk against 432 MFMAs per
//     wave and chunk) and written to LDS as TWO 16-bit images (hi | lo) in the bf16 kernel's layout;
//   * the weights are split once on the host (pack_conv3x3_split): per K-step one 16 KB unit = hi tile | lo tile, each already in
//     its swizzled LDS image, streamed by LDS-DMA into a 3-deep ring exactly as in the bf16 kernel.  f16 halves: the whole weight
//     tensor is scaled by a power of two so that max|w| sits at 2^10 (w_lo then stays clear of f16's subnormal range); the
//     epilogue multiplies the accumulators by the inverse (exact);
//   * LDS: 2 x (24 + 24) KB of A + 3 x 16 KB of B = 144 KB - one 512-thread workgroup per CU, two waves per SIMD, up to 256
//     VGPRs per wave (64 accumulators + 64 operand-fragment registers + 24 staging registers);
//   * epilogue: + bias, fp32 stores (per 16-pixel block one wave-private hop through the idle A buffer, then four stores of four whole
//     256-byte pixel rows each: +1.8 % on an f16x3 step against 16-byte stores straight from the accumulators), GroupNorm partial sums
//     in the bf16 kernel's slot layout (conv3x3_bf16_stats_slots applies).
// Roofline: MFMA.  3 x (2 * 9 * Cin * Cout) FLOP of 16-bit MFMA work per output pixel; counted as ALGORITHMIC flops (one product
// per multiply-add) the ceiling is 2.5 PF / 3 = 833 TFLOP/s.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "conv_common.hpp"

namespace srgd {
namespace {

constexpr int PH = 8, PW = 32;                 // output patch
constexpr int HP = PH + 2, WP = PW + 2;        // halo patch: 10 x 34 = 340 pixels
constexpr int KC = 32;                         // channels per chunk (64-byte rows of 16-bit values)
constexpr int BN3 = 128;
constexpr int NT3 = 512;
constexpr int A_IMG = 24 * 1024;               // one 16-bit halo image (340 px * 64 B = 21,760 used; 1,536 16-byte pieces)
constexpr int A_BUF = 2 * A_IMG;               // hi | lo
constexpr int B_TILE = BN3 * KC * 2;           // 8 KiB: one 16-bit weight tile
constexpr int B_SLOT = 2 * B_TILE;             // hi | lo
constexpr int LDS_BYTES = 2 * A_BUF + 3 * B_SLOT;   // 147,456: one workgroup per CU
constexpr int LDS1_BYTES = 2 * A_IMG + 3 * B_TILE;  // 73,728: the one-term instances (hi images alone)

struct Split3Args {
  const float* in0; const float* in1; int C0, C1;
  int B, H, W;
  const void* w;          // pack_conv3x3_split
  const float* bias;
  float w_inv_scale;      // 1 / (power-of-two weight scale)
  int Cout;
  float* out;
  float* gn_partial; int groups;
  const float* gn_in_a;   // GNIN: y = silu(a[b][c] * x + b[b][c]) applied to the input while it is staged ([B][Cin] fp32 each)
  const float* gn_in_b;
};

// One K-row of a K-step, for both kernels below: the wave's pixel block I (16 pixels) of tap `tap` against its four 16-channel weight
// fragments - twelve MFMAs, x_lo * w_hi, then x_hi * w_lo, then x_hi * w_hi into the same four accumulators.  A = the hi halo image
// in LDS, the lo image IMG bytes behind it; a_addr, mma, tap and the weight fragments bh0..3 / bl0..3 are the caller's.
#define SPLIT_K_ROW(A, IMG, I, C0_, C1_, C2_, C3_)                                             \
  {                                                                                            \
    const frag ah = *reinterpret_cast<const frag*>((A) + a_addr(tap, I));                      \
    const frag al = *reinterpret_cast<const frag*>((A) + (IMG) + a_addr(tap, I));              \
    mma(C0_, bh0, al); mma(C1_, bh1, al); mma(C2_, bh2, al); mma(C3_, bh3, al);                \
    mma(C0_, bl0, ah); mma(C1_, bl1, ah); mma(C2_, bl2, ah); mma(C3_, bl3, ah);                \
    mma(C0_, bh0, ah); mma(C1_, bh1, ah); mma(C2_, bh2, ah); mma(C3_, bh3, ah);                \
  }

// The one-term instances' K-row: x_hi * w_hi alone, four MFMAs.
#define HI_K_ROW(A, I, C0_, C1_, C2_, C3_)                                                     \
  {                                                                                            \
    const frag ah = *reinterpret_cast<const frag*>((A) + a_addr(tap, I));                      \
    mma(C0_, bh0, ah); mma(C1_, bh1, ah); mma(C2_, bh2, ah); mma(C3_, bh3, ah);                \
  }

// 8 fp32 (two 16-byte vectors) -> their 8 f16 hi halves, bit for bit the hi fragment of split8<true> (split_hi_f16: a finite value
// beyond f16's range saturates, a NaN or an infinity leaves as NaN); no lo halves are computed.
__device__ __forceinline__ void hi8(const u32x4& r0, const u32x4& r1, u32x4& hi) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned ua = k < 2 ? r0[2 * k] : r1[2 * k - 4], ub = k < 2 ? r0[2 * k + 1] : r1[2 * k - 3];   // (copied out first: conv_common.hpp)
    float a = __uint_as_float(ua), b = __uint_as_float(ub);
    f32x2 hf;
    const unsigned h = split_hi_f16(a, b, hf);
    hi[k] = h;
  }
}

// The lane's sixteen bias values (both kernels below): channels chw + chl .. + 15 (16-byte aligned: launcher), zero without a bias.
__device__ __forceinline__ void split_load_bias(const float* bias, int chw, int chl, f32x4& bs0, f32x4& bs1, f32x4& bs2, f32x4& bs3) {
  bs0 = bs1 = bs2 = bs3 = f32x4{0.f, 0.f, 0.f, 0.f};
  if (bias) {
    const float* bp = bias + chw + chl;
    bs0 = *reinterpret_cast<const f32x4*>(bp);
    bs1 = *reinterpret_cast<const f32x4*>(bp + 4);
    bs2 = *reinterpret_cast<const f32x4*>(bp + 8);
    bs3 = *reinterpret_cast<const f32x4*>(bp + 12);
  }
}

// (the (hi, lo) operand split split8<F16> and the GNIN transform act4: conv_common.hpp)
// GNIN instances: the PRODUCER's GroupNorm-apply + SiLU (reference Block.forward model.py:250-259 between two convolutions) is applied
// to the fp32 halo pieces in registers, ahead of the split - the separate gn_apply pass over that tensor (4 B read + 4 B written per
// element) disappears.  Out-of-image halo pixels stay zero (the convolution pads the ACTIVATED tensor).  v_exp_f32 / v_rcp_f32
// (1 ulp each) instead of gn_apply's expf and IEEE division: ~3e-7 relative, far inside the mode's 2^-22 per product.
//
// TERMS == 1 (f16 halves only; the engine's f16x1 mode): y = conv(hi(x), hi(w s)) / s + bias - ONE MFMA per fragment pair.  Same tile
// decode, staging, swizzled images, ring and epilogue; what exists for the lo halves is compiled out: the lo halo image (an A buffer
// is one 24 KB image), the lo weight tile's DMA (the hi tile of pack_conv3x3_split's unit is copied, the lo tile behind it in HBM is
// skipped; a ring slot is 8 KB), the lo fragment reads and eight of the twelve MFMAs of a K-row.  LDS 2 x 24 + 3 x 8 = 72 KB.
// Two workgroups would fit a CU's LDS but need 128 VGPRs per wave; the instances take 176 (198 with GNIN: 64 accumulators, 24 staging
// registers, 16 coefficients, 32 operand fragments, one operand address per tap and block) and a build held to 128 spills 64 .. 123 of
// them (compiled only, never timed: profiles/f16x1_bench.txt), so the kernel keeps the three-term kernel's bounds: one workgroup per CU, two waves per SIMD.
// (-DSRGD_SPLIT1_WAVES=4 compiles that build, for the resource table only - tools/time_f16x1.py prints it; the launcher stays as it is.)
#ifndef SRGD_SPLIT1_WAVES
#define SRGD_SPLIT1_WAVES 2
#endif
template <bool STATS, bool F16, bool GNIN, int TERMS = 3>
__global__ __launch_bounds__(NT3, TERMS == 1 ? SRGD_SPLIT1_WAVES : 2) void conv3x3_split_kernel(Split3Args p) {
  static_assert(TERMS == 3 || (TERMS == 1 && F16), "one term: f16 halves");
  constexpr bool ONE = TERMS == 1;
  constexpr int ABUF = ONE ? A_IMG : A_BUF;       // one A buffer in LDS
  constexpr int BSLOT = ONE ? B_TILE : B_SLOT;    // one ring slot in LDS (in HBM a unit is B_SLOT bytes for both)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int r16 = lane & 15, q16 = lane >> 4;

  // ---- tile coordinates (conv_common.hpp: XCD-aware remap - each XCD a contiguous band of tiles -, n-tiles fastest)
  int n_tiles, tiles_x, tiles_y, nt, b, trem, y0, x0;
  static_assert(PH == 8 && BN3 == 128, "patch_tile_decode and gn_partial_store: 8-row patches, 128-channel tiles");
  patch_tile_decode<PW>(blockIdx.x, p.Cout, p.W, p.H, p.B, n_tiles, tiles_x, tiles_y, nt, b, trem, y0, x0);
  const int Cin = p.C0 + p.C1;
  const int CC = Cin / KC;

  // ---- A staging: 1,536 16-byte LDS pieces per image (1,360 used); thread t owns pieces t, t + 512, t + 1024.  Piece g = halo
  // pixel P = g >> 2, stored chunk position g & 3, which holds SOURCE chunk (g & 3) ^ row_swz(P) (8 channels = 32 bytes of fp32).
  int a_pix0, a_pix1, a_pix2;
#define K_A_DECL(J)                                                           \
  {                                                                           \
    const int g = tid + NT3 * J;                                              \
    const int P = g >> 2;                                                     \
    const int py = P / WP, px = P - py * WP;                                  \
    const int y = y0 + py - 1, x = x0 + px - 1;                               \
    const bool ok = P < HP * WP && y >= 0 && y < p.H && x >= 0 && x < p.W;    \
    a_pix##J = ok ? y * p.W + x : -1;                                         \
  }
  K_A_DECL(0) K_A_DECL(1) K_A_DECL(2)
#undef K_A_DECL
  // (tid + 512 J) >> 2 = (tid >> 2) + 128 J and 128 J vanishes from row_swz: one source chunk for the three pieces
  const int a_sub = (tid & 3) ^ row_swz(tid >> 2);
  const size_t img_elems0 = (size_t)p.H * p.W * p.C0, img_elems1 = (size_t)p.H * p.W * p.C1;
  const __amdgpu_buffer_rsrc_t rs0 =
      __builtin_amdgcn_make_buffer_rsrc((void*)(p.in0 + (size_t)b * img_elems0), 0, (int)(img_elems0 * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.in1 ? p.in1 + (size_t)b * img_elems1 : p.in0), 0, p.in1 ? (int)(img_elems1 * 4) : 0, 0x00020000);
  const size_t w_tile_stride = (size_t)n_tiles * B_SLOT;              // bytes between consecutive (tap, cc) units
  const char* w_base = (const char*)p.w + (size_t)nt * B_SLOT;
  const __amdgpu_buffer_rsrc_t rsw =
      __builtin_amdgcn_make_buffer_rsrc((void*)w_base, 0, (int)((size_t)(9 * CC - 1) * w_tile_stride + B_SLOT), 0x00020000);

  char* const sA0 = smem;
  char* const sB0 = smem + 2 * ABUF;

  // fp32 halo pieces of the NEXT chunk in flight (24 registers)
  u32x4 ra00, ra01, ra10, ra11, ra20, ra21;
  auto load_piece = [&](int cc, int a_pix, u32x4& lo16, u32x4& hi16) {
    const int c = cc * KC;
    const bool first = c < p.C0;
    const int Cs = first ? p.C0 : p.C1;
    const int coff = first ? c : c - p.C0;
    const int voff = a_pix >= 0 ? (a_pix * Cs + coff + a_sub * 8) * 4 : 0x7ffffff0;
    if (first) {
      lo16 = __builtin_amdgcn_raw_buffer_load_b128(rs0, voff, 0, 0);
      hi16 = __builtin_amdgcn_raw_buffer_load_b128(rs0, voff, 16, 0);
    } else {
      lo16 = __builtin_amdgcn_raw_buffer_load_b128(rs1, voff, 0, 0);
      hi16 = __builtin_amdgcn_raw_buffer_load_b128(rs1, voff, 16, 0);
    }
  };
  f32x4 ga0, ga1, gb0, gb1;                        // GNIN: scale / shift of the thread's 8 channels of the chunk in flight
  auto load_a = [&](int cc) {
    load_piece(cc, a_pix0, ra00, ra01);
    load_piece(cc, a_pix1, ra10, ra11);
    load_piece(cc, a_pix2, ra20, ra21);
    if constexpr (GNIN) {                          // one source (launcher); the same 8 channels for all three pieces
      const float* ca = p.gn_in_a + (size_t)b * Cin + cc * KC + a_sub * 8;
      const float* cb = p.gn_in_b + (size_t)b * Cin + cc * KC + a_sub * 8;
      ga0 = *reinterpret_cast<const f32x4*>(ca); ga1 = *reinterpret_cast<const f32x4*>(ca + 4);
      gb0 = *reinterpret_cast<const f32x4*>(cb); gb1 = *reinterpret_cast<const f32x4*>(cb + 4);
    }
  };
  auto store_piece = [&](int cc, int j, u32x4 r0, u32x4 r1) {
    if constexpr (GNIN) {
      if ((j == 0 ? a_pix0 : (j == 1 ? a_pix1 : a_pix2)) >= 0) { act4(r0, ga0, gb0); act4(r1, ga1, gb1); }
    }
    if constexpr (ONE) {
      u32x4 hi;
      hi8(r0, r1, hi);
      *reinterpret_cast<u32x4*>(sA0 + (cc & 1) * ABUF + (tid + NT3 * j) * 16) = hi;
    } else {
      u32x4 hi, lo;
      split8<F16>(r0, r1, hi, lo);
      char* dst = sA0 + (cc & 1) * A_BUF + (tid + NT3 * j) * 16;
      *reinterpret_cast<u32x4*>(dst) = hi;
      *reinterpret_cast<u32x4*>(dst + A_IMG) = lo;
    }
  };
  // K-step (cc, tap) -> weight unit (tap, cc) into ring slot tap % 3 (9 % 3 == 0); every wave copies 1 KiB of the hi tile and
  // 1 KiB of the lo tile (one term: the hi tile alone - ONE request per K-step).  `tap` is a compile-time constant (0..10: 9 and 10
  // are taps 0 and 1 of the next chunk).
  const int w_tap_stride = (int)(CC * w_tile_stride);
  const int tid16 = tid * 16;
  auto issue_b = [&](int cc, int tap) {
    if (tap >= 9) { tap -= 9; cc += 1; }
    char* dst = sB0 + (tap % 3) * BSLOT + wave * 1024;
    const int so = tap * w_tap_stride + cc * (int)w_tile_stride;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_ptr)dst, 16, tid16, so, 0, 0);
    if constexpr (!ONE) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_ptr)(dst + B_TILE), 16, tid16, so + B_TILE, 0, 0);
  };

  f32x4 c00 = 0, c01 = 0, c02 = 0, c03 = 0, c10 = 0, c11 = 0, c12 = 0, c13 = 0,
        c20 = 0, c21 = 0, c22 = 0, c23 = 0, c30 = 0, c31 = 0, c32 = 0, c33 = 0;

  // operand addresses: conv3x3_bf16.hip's (weight row n = wn*64 + j*16 + r16, chunk q16; halo pixel P = lp + Pc)
  const int b_base = (wn * 64 + r16) * 64 + ((q16 ^ row_swz(r16)) << 4);
  const int lp = 2 * wm * WP + r16, lp8 = lp << 3, lp64 = lp * 64, q16s = q16 << 4;
  auto a_addr = [&](int tap, int i) {
    const int dy = tap / 3, dx = tap - dy * 3;
    const int Pc = ((i >> 1) + dy) * WP + (i & 1) * 16 + dx;
    return lp64 + (((lp8 + Pc * 8) & 0x30) ^ q16s) + Pc * 64;
  };
  typedef u32x4 frag;      // 8 x 16-bit
  auto mma = [&](f32x4& c, const frag& wt, const frag& px) {
    if constexpr (F16) c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, wt), __builtin_bit_cast(f16x8, px), c, 0, 0, 0);
    else c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wt), __builtin_bit_cast(bf16x8, px), c, 0, 0, 0);
  };
  auto compute = [&](int cc, int tap) {
    const char* A = sA0 + (cc & 1) * ABUF;
    const char* Bt = sB0 + (tap % 3) * BSLOT;
    const frag bh0 = *reinterpret_cast<const frag*>(Bt + b_base), bh1 = *reinterpret_cast<const frag*>(Bt + b_base + 1024),
               bh2 = *reinterpret_cast<const frag*>(Bt + b_base + 2048), bh3 = *reinterpret_cast<const frag*>(Bt + b_base + 3072);
    if constexpr (ONE) {
      HI_K_ROW(A, 0, c00, c01, c02, c03)
      HI_K_ROW(A, 1, c10, c11, c12, c13)
      HI_K_ROW(A, 2, c20, c21, c22, c23)
      HI_K_ROW(A, 3, c30, c31, c32, c33)
    } else {
      const frag bl0 = *reinterpret_cast<const frag*>(Bt + B_TILE + b_base), bl1 = *reinterpret_cast<const frag*>(Bt + B_TILE + b_base + 1024),
                 bl2 = *reinterpret_cast<const frag*>(Bt + B_TILE + b_base + 2048), bl3 = *reinterpret_cast<const frag*>(Bt + B_TILE + b_base + 3072);
      SPLIT_K_ROW(A, A_IMG, 0, c00, c01, c02, c03)
      SPLIT_K_ROW(A, A_IMG, 1, c10, c11, c12, c13)
      SPLIT_K_ROW(A, A_IMG, 2, c20, c21, c22, c23)
      SPLIT_K_ROW(A, A_IMG, 3, c30, c31, c32, c33)
    }
  };

  // ---- prologue: A(0) through registers, B[0], B[1]
  issue_b(0, 0);
  issue_b(0, 1);
  load_a(0);
  store_piece(0, 0, ra00, ra01);
  store_piece(0, 1, ra10, ra11);
  store_piece(0, 2, ra20, ra21);
  if constexpr (ONE) WAIT_VM(1); else WAIT_VM(2);  // B[0] landed (B[1]'s two copies - one term: its one copy - may still fly)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BARRIER();

  // ---- main loop.  Per K-step s = (cc, tap): issue B[s+2]; tap 0 additionally issues the six fp32 loads of chunk cc+1 (after the
  // weight copies: they are then younger than B[s+2] and the counted waits of taps 0 and 1 let them fly); compute(s); taps 3..5 split
  // one piece each into the other A buffer; wait until B[s+1] has landed; barrier.
  // vmcnt bookkeeping (loads retire in order): at the end of tap t the requests younger than B[s+1] are
  //   tap 0: B[s+2] (2) + A (6) = 8;   tap 1: A (6) + B[s+2] (2) = 8;   taps 2..8: B[s+2] (2)   (tap 2's wait retires the A loads);
  //   GNIN: the chunk's four coefficient loads ride with the A loads (12 instead of 8).
  // One term: B[s+2] is ONE request (the hi tile), so
  //   tap 0: B[s+2] (1) + A (6) = 7;   tap 1: A (6) + B[s+2] (1) = 7;   taps 2..8: B[s+2] (1);   GNIN: 11 instead of 7;
  //   prologue: B[1] (1) behind B[0] (the A loads, younger, were drained by the stores that consumed them);
  //   last chunk: taps 0..6 B[s+2] (1), taps 7 and 8 nothing in flight (0).
  for (int cc = 0; cc < CC - 1; ++cc) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      issue_b(cc, tap + 2);
      if (tap == 0) {
        __builtin_amdgcn_sched_barrier(0);         // the six loads stay BEHIND the weight copies (the counted waits assume it)
        load_a(cc + 1);
        __builtin_amdgcn_sched_barrier(0);
      }
      compute(cc, tap);
      if (tap == 3) store_piece(cc + 1, 0, ra00, ra01);
      if (tap == 4) store_piece(cc + 1, 1, ra10, ra11);
      if (tap == 5) store_piece(cc + 1, 2, ra20, ra21);
      if constexpr (ONE) {
        if (tap < 2) { if constexpr (GNIN) WAIT_VM(11); else WAIT_VM(7); }
        else WAIT_VM(1);
      } else {
        if (tap < 2) { if constexpr (GNIN) WAIT_VM(12); else WAIT_VM(8); }        // GNIN: + the four coefficient loads of tap 0
        else WAIT_VM(2);
      }
      if (tap == 8) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // this wave's A pieces are in LDS before the barrier publishes them
      BARRIER();
    }
  }
  {
    const int cc = CC - 1;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      if (tap < 7) issue_b(cc, tap + 2);
      compute(cc, tap);
      if (tap >= 7) WAIT_VM(0); else if constexpr (ONE) WAIT_VM(1); else WAIT_VM(2);
      if (tap < 8) BARRIER();
    }
  }

  // ------------------------------- epilogue (register-direct, fp32) --------------------------
  // Accumulator block (mi, J), register e of lane (r16, g) = pixel (patch row 2 wm + (mi >> 1), x = 16 (mi & 1) + r16), output channel
  // 64 wn + 16 g + 4 J + e (regepi_row_channel): a lane's sixteen registers of a pixel block are 16 consecutive channels = 64 bytes.
  const int chw = nt * BN3 + wn * 64;
  const int chl = q16 * 16;
  f32x4 bs0, bs1, bs2, bs3;
  split_load_bias(p.bias, chw, chl, bs0, bs1, bs2, bs3);
  const u32x4 rso = make_raw_rsrc(p.out + ((size_t)(b * p.H + y0 + 2 * wm) * p.W + x0) * p.Cout + chw, (unsigned)(2 * p.W * p.Cout * 4));
  const int o_voff = (r16 * p.Cout + chl) * 4;
  // Stores leave as full lines (the wave's 64 fp32 channels of a pixel = 256 bytes): each 16-pixel block goes through 16 staging rows
  // of the wave (272-byte pitch) in the A buffer the last chunk does not use, and every store instruction then writes four whole
  // pixel rows instead of 64 scattered 16-byte pieces (conv3x3_bf16.hip; wave-private, no barrier, compiler fences only).
  constexpr int STG_ROW = 272;
  static_assert(8 * 16 * STG_ROW <= A_BUF, "store staging fits the idle A buffer");
  // One term: the idle A buffer is one 24 KB image and holds five waves' rows; waves 5..7 stage in ring slots 0 and 1, which nobody
  // reads any more: a wave arrives here past tap 7's barrier, so every wave has finished taps 6 and 7 (slots 0 and 1), every copy has
  // landed (tap 7's vmcnt(0)), and tap 8, which others may still be computing, reads slot 2 and the OTHER A buffer.
  static_assert(5 * 16 * STG_ROW <= A_IMG && 3 * 16 * STG_ROW <= 2 * B_TILE, "one term: store staging fits the idle A image + two ring slots");
  char* const stg = ONE ? (wave < 5 ? smem + (CC & 1) * ABUF + wave * (16 * STG_ROW) : sB0 + (wave - 5) * (16 * STG_ROW))
                        : smem + (CC & 1) * ABUF + wave * (16 * STG_ROW);
  const int stg_w = r16 * STG_ROW + q16 * 64;
  const int stg_r = (lane >> 4) * STG_ROW + (lane & 15) * 16;       // read-back: pixel lane >> 4 (+ 4, 8, 12), 16-byte piece lane & 15
  const int line_off = (lane >> 4) * p.Cout * 4 + (lane & 15) * 16;
  const float ws = p.w_inv_scale;
  f32x4 s1v = {0.f, 0.f, 0.f, 0.f}, s2v = s1v;
  asm volatile("" : "+v"(bs0), "+v"(bs1), "+v"(bs2), "+v"(bs3));
#define K_EMIT(MI, C0_, C1_, C2_, C3_)                                                          \
  do {                                                                                             \
    const int so_ = ((((MI) >> 1) * p.W + ((MI) & 1) * 16) * p.Cout) * 4;                          \
    const f32x4 v0 = C0_ * ws + bs0, v1 = C1_ * ws + bs1, v2 = C2_ * ws + bs2, v3 = C3_ * ws + bs3; \
    if (STATS) {                                                                                   \
      s1v += (v0 + v1) + (v2 + v3);                                                                \
      s2v = __builtin_elementwise_fma(v0, v0, s2v);                                                \
      s2v = __builtin_elementwise_fma(v1, v1, s2v);                                                \
      s2v = __builtin_elementwise_fma(v2, v2, s2v);                                                \
      s2v = __builtin_elementwise_fma(v3, v3, s2v);                                                \
    }                                                                                              \
    {                                                                                              \
      *reinterpret_cast<f32x4*>(stg + stg_w) = v0;                                                 \
      *reinterpret_cast<f32x4*>(stg + stg_w + 16) = v1;                                            \
      *reinterpret_cast<f32x4*>(stg + stg_w + 32) = v2;                                            \
      *reinterpret_cast<f32x4*>(stg + stg_w + 48) = v3;                                            \
      asm volatile("" ::: "memory");                                                               \
      const u32x4 w0_ = *reinterpret_cast<const u32x4*>(stg + stg_r);                              \
      const u32x4 w1_ = *reinterpret_cast<const u32x4*>(stg + stg_r + 4 * STG_ROW);                \
      const u32x4 w2_ = *reinterpret_cast<const u32x4*>(stg + stg_r + 8 * STG_ROW);                \
      const u32x4 w3_ = *reinterpret_cast<const u32x4*>(stg + stg_r + 12 * STG_ROW);               \
      asm volatile("" ::: "memory");                                                               \
      buffer_store16(w0_, rso, line_off, so_);                                                     \
      buffer_store16(w1_, rso, line_off, so_ + 4 * p.Cout * 4);                                    \
      buffer_store16(w2_, rso, line_off, so_ + 8 * p.Cout * 4);                                    \
      buffer_store16(w3_, rso, line_off, so_ + 12 * p.Cout * 4);                                   \
    }                                                                                              \
  } while (0)
  K_EMIT(0, c00, c01, c02, c03);
  K_EMIT(1, c10, c11, c12, c13);
  K_EMIT(2, c20, c21, c22, c23);
  K_EMIT(3, c30, c31, c32, c33);
#undef K_EMIT
  if (STATS) gn_partial_store<BN3, 4>(s1v, s2v, p.Cout, p.groups, p.gn_partial, r16, q16, wave, wm, tiles_y, tiles_x, trem, nt, b, chw, chl);
}


// ---- the two-workgroups-per-CU form -----------------------------------------------------------------------------------------------
// Same arithmetic, LDS images and weight stream; the tile is an 8 x 16 pixel patch (M = 128) x 128 channels on 256 threads (4 waves,
// 2 along M x 2 along N, each still 64 pixels x 64 channels = 4 patch rows of 16), the A image is SINGLE-buffered (hi | lo, 24 KB;
// the next chunk's pieces wait in registers and are split + written at the chunk boundary, between two barriers) and the weight ring
// stays 3 deep: 72 KB per workgroup - TWO workgroups per CU.  Why: with one workgroup per CU every barrier of the K loop (one per
// K-step) leaves the matrix pipe idle until the first operand fragments are back from LDS, and so do the prologue, the chunk boundary
// and the epilogue; a second, independent workgroup on the same SIMDs fills those gaps (the bf16 kernel's arrangement).  Price: the
// weight stream is fetched per 128 pixels instead of per 256 (L2 -> LDS), the halo overhead rises from 1.33 to 1.41.
constexpr int PW2 = 16, WP2 = PW2 + 2;            // halo patch 10 x 18 = 180 pixels
constexpr int NT2 = 256;
constexpr int A_IMG2 = 12 * 1024;                 // 768 16-byte pieces (720 used)
constexpr int A_BUF2 = 2 * A_IMG2;                // hi | lo
constexpr int LDS2_BYTES = A_BUF2 + 3 * B_SLOT;   // 73,728: two workgroups per CU

template <bool STATS, bool GNIN>
__global__ __launch_bounds__(NT2, 2) void conv3x3_split2_kernel(Split3Args p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int r16 = lane & 15, q16 = lane >> 4;

  // ---- tile coordinates (conv_common.hpp: XCD-aware remap - each XCD a contiguous band of tiles -, n-tiles fastest)
  int n_tiles, tiles_x, tiles_y, nt, b, trem, y0, x0;
  static_assert(PH == 8 && BN3 == 128, "patch_tile_decode and gn_partial_store: 8-row patches, 128-channel tiles");
  patch_tile_decode<PW2>(blockIdx.x, p.Cout, p.W, p.H, p.B, n_tiles, tiles_x, tiles_y, nt, b, trem, y0, x0);
  const int Cin = p.C0 + p.C1;
  const int CC = Cin / KC;

  // ---- A staging: 768 pieces per image (720 used); thread t owns pieces t, t + 256, t + 512 (same source chunk for all three)
  int a_pix0, a_pix1, a_pix2;
#define K_A_DECL(J)                                                           \
  {                                                                           \
    const int g = tid + NT2 * J;                                              \
    const int P = g >> 2;                                                     \
    const int py = P / WP2, px = P - py * WP2;                                \
    const int y = y0 + py - 1, x = x0 + px - 1;                               \
    const bool ok = P < HP * WP2 && y >= 0 && y < p.H && x >= 0 && x < p.W;   \
    a_pix##J = ok ? y * p.W + x : -1;                                         \
  }
  K_A_DECL(0) K_A_DECL(1) K_A_DECL(2)
#undef K_A_DECL
  const int a_sub = (tid & 3) ^ row_swz(tid >> 2);
  const size_t img_elems0 = (size_t)p.H * p.W * p.C0, img_elems1 = (size_t)p.H * p.W * p.C1;
  const __amdgpu_buffer_rsrc_t rs0 =
      __builtin_amdgcn_make_buffer_rsrc((void*)(p.in0 + (size_t)b * img_elems0), 0, (int)(img_elems0 * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(p.in1 ? p.in1 + (size_t)b * img_elems1 : p.in0), 0, p.in1 ? (int)(img_elems1 * 4) : 0, 0x00020000);
  const size_t w_tile_stride = (size_t)n_tiles * B_SLOT;
  const char* w_base = (const char*)p.w + (size_t)nt * B_SLOT;
  const __amdgpu_buffer_rsrc_t rsw =
      __builtin_amdgcn_make_buffer_rsrc((void*)w_base, 0, (int)((size_t)(9 * CC - 1) * w_tile_stride + B_SLOT), 0x00020000);

  char* const sA = smem;
  char* const sB0 = smem + A_BUF2;

  // (load_piece and load_a repeat conv3x3_split_kernel's: as functions shared by the two kernels they compiled to other instructions
  // in both - profiles/conv_common_refactor.txt)
  u32x4 ra00, ra01, ra10, ra11, ra20, ra21;
  f32x4 ga0, ga1, gb0, gb1;
  auto load_piece = [&](int cc, int a_pix, u32x4& lo16, u32x4& hi16) {
    const int c = cc * KC;
    const bool first = c < p.C0;
    const int Cs = first ? p.C0 : p.C1;
    const int coff = first ? c : c - p.C0;
    const int voff = a_pix >= 0 ? (a_pix * Cs + coff + a_sub * 8) * 4 : 0x7ffffff0;
    if (first) {
      lo16 = __builtin_amdgcn_raw_buffer_load_b128(rs0, voff, 0, 0);
      hi16 = __builtin_amdgcn_raw_buffer_load_b128(rs0, voff, 16, 0);
    } else {
      lo16 = __builtin_amdgcn_raw_buffer_load_b128(rs1, voff, 0, 0);
      hi16 = __builtin_amdgcn_raw_buffer_load_b128(rs1, voff, 16, 0);
    }
  };
  auto load_a = [&](int cc) {
    load_piece(cc, a_pix0, ra00, ra01);
    load_piece(cc, a_pix1, ra10, ra11);
    load_piece(cc, a_pix2, ra20, ra21);
    if constexpr (GNIN) {
      const float* ca = p.gn_in_a + (size_t)b * Cin + cc * KC + a_sub * 8;
      const float* cb = p.gn_in_b + (size_t)b * Cin + cc * KC + a_sub * 8;
      ga0 = *reinterpret_cast<const f32x4*>(ca); ga1 = *reinterpret_cast<const f32x4*>(ca + 4);
      gb0 = *reinterpret_cast<const f32x4*>(cb); gb1 = *reinterpret_cast<const f32x4*>(cb + 4);
    }
  };
  auto store_piece = [&](int j, u32x4 r0, u32x4 r1) {
    if constexpr (GNIN) {
      if ((j == 0 ? a_pix0 : (j == 1 ? a_pix1 : a_pix2)) >= 0) { act4(r0, ga0, gb0); act4(r1, ga1, gb1); }
    }
    u32x4 hi, lo;
    split8<true>(r0, r1, hi, lo);
    char* dst = sA + (tid + NT2 * j) * 16;
    *reinterpret_cast<u32x4*>(dst) = hi;
    *reinterpret_cast<u32x4*>(dst + A_IMG2) = lo;
  };
  // weight unit of K-step (cc, tap) -> ring slot tap % 3; every wave copies 2 x 1 KiB of the hi tile and 2 x 1 KiB of the lo tile
  const int w_tap_stride = (int)(CC * w_tile_stride);
  const int tid16 = tid * 16;
  auto issue_b = [&](int cc, int tap) {
    if (tap >= 9) { tap -= 9; cc += 1; }
    char* dst = sB0 + (tap % 3) * B_SLOT + wave * 1024;
    const int so = tap * w_tap_stride + cc * (int)w_tile_stride;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_ptr)dst, 16, tid16, so, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_ptr)(dst + 4096), 16, tid16, so + 4096, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_ptr)(dst + B_TILE), 16, tid16, so + B_TILE, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_ptr)(dst + B_TILE + 4096), 16, tid16, so + B_TILE + 4096, 0, 0);
  };

  f32x4 c00 = 0, c01 = 0, c02 = 0, c03 = 0, c10 = 0, c11 = 0, c12 = 0, c13 = 0,
        c20 = 0, c21 = 0, c22 = 0, c23 = 0, c30 = 0, c31 = 0, c32 = 0, c33 = 0;
  const int b_base = (wn * 64 + r16) * 64 + ((q16 ^ row_swz(r16)) << 4);
  // the wave's pixel block i (0..3) = patch row 4 wm + i, x = r16: halo pixel P = lp + Pc, lp = 4 wm WP2 + r16, Pc = (i + dy) WP2 + dx
  const int lp = 4 * wm * WP2 + r16, lp8 = lp << 3, lp64 = lp * 64, q16s = q16 << 4;
  auto a_addr = [&](int tap, int i) {
    const int dy = tap / 3, dx = tap - dy * 3;
    const int Pc = (i + dy) * WP2 + dx;
    return lp64 + (((lp8 + Pc * 8) & 0x30) ^ q16s) + Pc * 64;
  };
  typedef u32x4 frag;
  auto mma = [&](f32x4& c, const frag& wt, const frag& px) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, wt), __builtin_bit_cast(f16x8, px), c, 0, 0, 0);
  };
  auto compute = [&](int tap) {
    const char* Bt = sB0 + (tap % 3) * B_SLOT;
    const frag bh0 = *reinterpret_cast<const frag*>(Bt + b_base), bh1 = *reinterpret_cast<const frag*>(Bt + b_base + 1024),
               bh2 = *reinterpret_cast<const frag*>(Bt + b_base + 2048), bh3 = *reinterpret_cast<const frag*>(Bt + b_base + 3072);
    const frag bl0 = *reinterpret_cast<const frag*>(Bt + B_TILE + b_base), bl1 = *reinterpret_cast<const frag*>(Bt + B_TILE + b_base + 1024),
               bl2 = *reinterpret_cast<const frag*>(Bt + B_TILE + b_base + 2048), bl3 = *reinterpret_cast<const frag*>(Bt + B_TILE + b_base + 3072);
    SPLIT_K_ROW(sA, A_IMG2, 0, c00, c01, c02, c03)
    SPLIT_K_ROW(sA, A_IMG2, 1, c10, c11, c12, c13)
    SPLIT_K_ROW(sA, A_IMG2, 2, c20, c21, c22, c23)
    SPLIT_K_ROW(sA, A_IMG2, 3, c30, c31, c32, c33)
  };

  // ---- prologue
  issue_b(0, 0);
  issue_b(0, 1);
  load_a(0);
  store_piece(0, ra00, ra01);
  store_piece(1, ra10, ra11);
  store_piece(2, ra20, ra21);
  WAIT_VM(4);                                    // B[0] landed (B[1]'s four copies may still fly)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  BARRIER();

  // ---- main loop.  vmcnt bookkeeping: B[s+2] is four requests, the A loads six (+ four coefficient loads with GNIN), all of them
  // younger than B[s+1] at the end of taps 0 and 1; tap 2's wait (4) retires them.  At the chunk boundary (after tap 8's barrier:
  // every wave has finished reading the A image) the next chunk's pieces are split and written, then a second barrier publishes them.
  for (int cc = 0; cc < CC - 1; ++cc) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      issue_b(cc, tap + 2);
      if (tap == 0) {
        __builtin_amdgcn_sched_barrier(0);
        load_a(cc + 1);
        __builtin_amdgcn_sched_barrier(0);
      }
      compute(tap);
      if (tap < 2) { if constexpr (GNIN) WAIT_VM(14); else WAIT_VM(10); }
      else WAIT_VM(4);
      BARRIER();
      if (tap == 8) {
        store_piece(0, ra00, ra01);
        store_piece(1, ra10, ra11);
        store_piece(2, ra20, ra21);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        BARRIER();
      }
    }
  }
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    if (tap < 7) issue_b(CC - 1, tap + 2);
    compute(tap);
    if (tap < 7) WAIT_VM(4); else WAIT_VM(0);
    if (tap < 8) BARRIER();
  }

  // ---- epilogue (register-direct, fp32): block mi = patch row 4 wm + mi, pixel x = r16, channels 64 wn + 16 g + 4 J + e
  const int chw = nt * BN3 + wn * 64;
  const int chl = q16 * 16;
  f32x4 bs0, bs1, bs2, bs3;
  split_load_bias(p.bias, chw, chl, bs0, bs1, bs2, bs3);
  const u32x4 rso = make_raw_rsrc(p.out + ((size_t)(b * p.H + y0 + 4 * wm) * p.W + x0) * p.Cout + chw, (unsigned)(4 * p.W * p.Cout * 4));
  const int o_voff = (r16 * p.Cout + chl) * 4;
  const float ws = p.w_inv_scale;
  f32x4 s1v = {0.f, 0.f, 0.f, 0.f}, s2v = s1v;
  asm volatile("" : "+v"(bs0), "+v"(bs1), "+v"(bs2), "+v"(bs3));
#define K_EMIT(MI, C0_, C1_, C2_, C3_)                                                          \
  do {                                                                                             \
    const int so_ = ((MI) * p.W * p.Cout) * 4;                                                     \
    const f32x4 v0 = C0_ * ws + bs0, v1 = C1_ * ws + bs1, v2 = C2_ * ws + bs2, v3 = C3_ * ws + bs3; \
    if (STATS) {                                                                                   \
      s1v += (v0 + v1) + (v2 + v3);                                                                \
      s2v = __builtin_elementwise_fma(v0, v0, s2v);                                                \
      s2v = __builtin_elementwise_fma(v1, v1, s2v);                                                \
      s2v = __builtin_elementwise_fma(v2, v2, s2v);                                                \
      s2v = __builtin_elementwise_fma(v3, v3, s2v);                                                \
    }                                                                                              \
    buffer_store16(__builtin_bit_cast(u32x4, v0), rso, o_voff, so_);                               \
    buffer_store16(__builtin_bit_cast(u32x4, v1), rso, o_voff, so_ + 16);                          \
    buffer_store16(__builtin_bit_cast(u32x4, v2), rso, o_voff, so_ + 32);                          \
    buffer_store16(__builtin_bit_cast(u32x4, v3), rso, o_voff, so_ + 48);                          \
  } while (0)
  K_EMIT(0, c00, c01, c02, c03);
  K_EMIT(1, c10, c11, c12, c13);
  K_EMIT(2, c20, c21, c22, c23);
  K_EMIT(3, c30, c31, c32, c33);
#undef K_EMIT
  // twice the patches of the 512-thread kernel with half the waves each: the same slot count (conv3x3_stats_slots)
  if (STATS) gn_partial_store<BN3, 2>(s1v, s2v, p.Cout, p.groups, p.gn_partial, r16, q16, wave, wm, tiles_y, tiles_x, trem, nt, b, chw, chl);
}

}  // namespace

bool conv3x3_split_eligible(const ConvArgs& a) { return conv3x3_patch_eligible(a, 4, B_SLOT); }

// ---- host-side split of the weights ---------------------------------------------------------------------------------------------
// f16: round-to-nearest-even conversion of a float (finite, |x| < 65520) to IEEE binary16 bits, subnormals kept.
unsigned short f32_to_f16_host(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  const uint32_t au = u & 0x7fffffffu;
  if (au >= 0x7f800000u) return (unsigned short)(sign | (au > 0x7f800000u ? 0x7e00u : 0x7c00u));
  if (au >= 0x477ff000u) return (unsigned short)(sign | 0x7c00u);           // >= 65520 rounds to infinity
  if (au < 0x33000001u) return (unsigned short)sign;                        // <= 2^-25: rounds to zero
  int e = (int)(au >> 23) - 127;
  uint32_t m = (au & 0x7fffffu) | 0x800000u;                                // 24-bit significand
  int shift;                                                                // bits to drop
  uint32_t base;
  if (e >= -14) { shift = 13; base = (uint32_t)(e + 15) << 10; m &= 0x7fffffu; }
  else { shift = 13 + (-14 - e); base = 0; }                                // subnormal: keep the leading bit in m
  const uint32_t keep = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
  uint32_t h = base + keep;
  if (rem > half || (rem == half && (keep & 1u))) h += 1;                   // carries into the exponent correctly
  return (unsigned short)(sign | h);
}
float f16_bits_to_f32(unsigned short h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  const int e = (h >> 10) & 31;
  const uint32_t m = h & 0x3ffu;
  float v;
  if (e == 0) v = std::ldexp((float)m, -24);
  else if (e == 31) v = m ? NAN : INFINITY;
  else v = std::ldexp((float)(m | 0x400u), e - 25);
  uint32_t u;
  std::memcpy(&u, &v, 4);
  u |= sign;
  std::memcpy(&v, &u, 4);
  return v;
}
float bf16_bits_to_f32(unsigned short h) {
  const uint32_t u = (uint32_t)h << 16;
  float v;
  std::memcpy(&v, &u, 4);
  return v;
}

// The weight scale of a layer: the power of two that puts max|w| into [2^10, 2^11) for f16 halves (w_lo = w - w_hi then sits at
// 2^-1 or above for the largest weights and loses nothing to f16's subnormal spacing of 2^-24 until |w| is 2^-13 of the maximum);
// 1 for bf16 halves (fp32's exponent range).
float split_weight_scale(const float* w, size_t n, bool f16) {
  if (!f16) return 1.0f;
  float m = 0.f;
  for (size_t i = 0; i < n; ++i) m = std::max(m, std::fabs(w[i]));
  if (!(m > 0.f) || !std::isfinite(m)) return 1.0f;
  int e;
  (void)std::frexp(m, &e);                       // m = f * 2^e, f in [0.5, 1)  ->  floor(log2 m) = e - 1
  return std::ldexp(1.0f, 10 - (e - 1));
}
void split_halves_host(float v, bool f16, unsigned short* hi, unsigned short* lo) {
  if (f16) {
    *hi = f32_to_f16_host(v);
    *lo = f32_to_f16_host(v - f16_bits_to_f32(*hi));
  } else {
    *hi = f32_to_bf16_host(v);
    *lo = f32_to_bf16_host(v - bf16_bits_to_f32(*hi));
  }
}

// OIHW fp32 -> [tap][cc][ntile][hi tile | lo tile], each tile 128 rows x 64 B in conv3x3_bf16's swizzled LDS image and row order
void pack_conv3x3_split(const float* src_oihw, int Cin, int Cout, bool f16, float scale, std::vector<unsigned short>& out) {
  out.assign((size_t)9 * (Cin / KC) * (Cout / BN3) * 2 * BN3 * KC, 0);
  conv3x3_weight_walk(src_oihw, Cin, Cout, [&](size_t tile, int, int, int pos, float v) {
    unsigned short* hi_t = out.data() + tile * 2 * BN3 * KC;
    split_halves_host(v * scale, f16, &hi_t[pos], &hi_t[BN3 * KC + pos]);
  });
}

int conv3x3_split(const ConvArgs& a, const void* packed_w, float w_inv_scale, bool f16, hipStream_t st, const float* gn_in_a,
                  const float* gn_in_b, int form, int terms) {
  if (!conv3x3_split_eligible(a)) SRGD_FAIL("conv3x3_split: shape not eligible");
  if (terms != 3 && (terms != 1 || !f16)) SRGD_FAIL("conv3x3_split: three terms, or one term on f16 halves");
  const bool gnin = gn_in_a != nullptr;
  if (gnin && (a.C1 != 0 || !gn_in_b || !f16 || ((size_t)gn_in_a & 15) || ((size_t)gn_in_b & 15)))
    SRGD_FAIL("conv3x3_split: fused input GroupNorm needs one source, f16 halves and 16-byte aligned scale / shift arrays");
  if (a.bias && ((size_t)a.bias & 15)) SRGD_FAIL("conv3x3_split: the bias array must be 16-byte aligned");
  Split3Args p;
  p.in0 = (const float*)a.in0; p.in1 = (const float*)a.in1; p.C0 = a.C0; p.C1 = a.C1;
  p.B = a.B; p.H = a.Hin; p.W = a.Win; p.w = packed_w; p.bias = a.bias; p.w_inv_scale = w_inv_scale; p.Cout = a.Cout;
  p.out = (float*)a.out; p.gn_partial = a.gn_partial; p.groups = a.groups;
  p.gn_in_a = gn_in_a; p.gn_in_b = gn_in_b;
  const int grid = a.B * (a.Hin / PH) * (a.Win / PW) * (a.Cout / BN3);
  static bool attr_set[64] = {};
  if (DeviceSetup once(attr_set); once.need) {
#define K_SET(S_, F_, G_)                                                                              \
  SRGD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_split_kernel<S_, F_, G_>),          \
                               hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    K_SET(true, true, false) K_SET(false, true, false) K_SET(true, false, false) K_SET(false, false, false)
    K_SET(true, true, true) K_SET(false, true, true)
#undef K_SET
    once.done();
  }
  const bool stats = a.gn_partial != nullptr;
  if (terms == 1) {
    static bool attr_set1[64] = {};
    if (DeviceSetup once(attr_set1); once.need) {
#define K_SET1(S_, G_)                                                                                    \
  SRGD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_split_kernel<S_, true, G_, 1>),     \
                               hipFuncAttributeMaxDynamicSharedMemorySize, LDS1_BYTES));
      K_SET1(true, false) K_SET1(false, false) K_SET1(true, true) K_SET1(false, true)
#undef K_SET1
      once.done();
    }
#define K_GO1(S_, G_) hipLaunchKernelGGL((conv3x3_split_kernel<S_, true, G_, 1>), dim3(grid), dim3(NT3), LDS1_BYTES, st, p)
    if (stats && gnin) K_GO1(true, true); else if (stats) K_GO1(true, false); else if (gnin) K_GO1(false, true); else K_GO1(false, false);
#undef K_GO1
    SRGD_HIP(hipGetLastError());
    return 0;
  }
  // default: the 512-thread kernel (one workgroup per CU); SRGD_SPLIT3_WG=2: the 256-thread kernel (two per CU; f16 halves only).
  // Same-box A/B (profiles/r6/conv3x3_split_forms_ab.txt): bit-identical results, 0.3873 vs 0.3854 HR tiles/s - the kernel is not
  // waiting on its barriers, it runs at the matrix pipe's sustained rate like conv3x3_bf16 - so the form with half the weight traffic stays
  static const int env_form = env_int("SRGD_SPLIT3_WG", 1);
  const int wg_form = form ? form : env_form;
  if (f16 && wg_form != 1) {
    static bool attr_set2[64] = {};
    if (DeviceSetup once(attr_set2); once.need) {
#define K_SET2(S_, G_) SRGD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_split2_kernel<S_, G_>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS2_BYTES));
      K_SET2(true, false) K_SET2(false, false) K_SET2(true, true) K_SET2(false, true)
#undef K_SET2
      once.done();
    }
    const int grid2 = a.B * (a.Hin / PH) * (a.Win / PW2) * (a.Cout / BN3);
#define K_GO2(S_, G_) hipLaunchKernelGGL((conv3x3_split2_kernel<S_, G_>), dim3(grid2), dim3(NT2), LDS2_BYTES, st, p)
    if (stats && gnin) K_GO2(true, true); else if (stats) K_GO2(true, false); else if (gnin) K_GO2(false, true); else K_GO2(false, false);
#undef K_GO2
    SRGD_HIP(hipGetLastError());
    return 0;
  }
#define K_GO(S_, F_, G_) hipLaunchKernelGGL((conv3x3_split_kernel<S_, F_, G_>), dim3(grid), dim3(NT3), LDS_BYTES, st, p)
  if (gnin) { if (stats) K_GO(true, true, true); else K_GO(false, true, true); }
  else if (stats && f16) K_GO(true, true, false); else if (stats) K_GO(true, false, false);
  else if (f16) K_GO(false, true, false); else K_GO(false, false, false);
#undef K_GO
  SRGD_HIP(hipGetLastError());
  return 0;
}

}  // namespace srgd
