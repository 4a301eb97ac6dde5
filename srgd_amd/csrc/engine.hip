// Engine behind the C ABI of include/srgd_hip.h: owns the packed weights, the activation
// pool and the launch sequence of one ConditionalSRUnet evaluation (reference
// model.py:678-725) and of one tiled DDPM step (model.py:3346-3396) on a single HIP stream.
// No host synchronisation, no allocation after the first call with a given shape.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "../../include/srgd_hip.h"
#include "../../include/srgd_hip_kernels.h"
#include "kernels.hpp"

namespace srgd {
static thread_local std::string g_err;
void set_error(const std::string& m) { g_err = m; }
const char* last_error() { return g_err.c_str(); }

// float -> OCP fp8 e4m3 "fn" (4 exponent bits, bias 7, 3 mantissa bits, max 448, no infinity) -> float,
// round-to-nearest-even, saturating.  Subnormals of the format (multiples of 2^-9) are kept.
float round_through_e4m3(float x) {
  if (std::isnan(x)) return x;
  const float ax = std::fabs(x);
  if (ax >= 464.0f) return std::copysign(448.0f, x);        // halfway between 448 and the (absent) next value 480
  if (ax < 0x1p-10f) return std::copysign(0.0f, x);          // below half of the smallest subnormal 2^-9
  int ex;
  (void)std::frexp(ax, &ex);                                 // ax = m * 2^ex, m in [0.5, 1)
  int e = ex - 1;                                            // exponent of the leading bit
  if (e < -6) e = -6;                                        // subnormal range shares the quantum of 2^-6
  const float quantum = std::ldexp(1.0f, e - 3);             // 3 mantissa bits
  float q = std::nearbyint(ax / quantum) * quantum;          // default rounding mode: nearest even
  if (q > 448.0f) q = 448.0f;
  return std::copysign(q, x);
}

unsigned short f32_to_bf16_host(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// OIHW fp32 -> [tap][CoutPad][Cin] in the activation type (k contiguous), see conv_igemm.hip.
//   kind 1 (Downsample, model.py:106-110): the 1x1 conv over 'b (c p1 p2) h w' becomes a 2x2/stride-2 conv.
//   kind 2 (PixelShuffleUpsample, model.py:70-98): output columns are permuted to (i*2+j)*Cout/4 + ch so the
//   epilogue's pixel-shuffled stores are channel-contiguous.
void pack_conv_weights(const float* src, const float* bias_in, int kind, int Cin, int Cout, int CoutPad, int KS,
                       bool to_bf16, std::vector<unsigned char>& packed_out, std::vector<float>& bias_out) {
  const int taps = KS * KS;
  const size_t n = (size_t)taps * CoutPad * Cin;
  std::vector<float> packed(n, 0.f);
  bias_out.assign(Cout, 0.f);
  for (int o = 0; o < Cout; ++o) {
    int no = o;
    if (kind == 2) {
      const int ch = o >> 2, ij = o & 3;
      no = ij * (Cout >> 2) + ch;
    }
    if (bias_in) bias_out[no] = bias_in[o];
    for (int t = 0; t < taps; ++t) {
      const int dy = t / KS, dx = t - dy * KS;
      for (int i = 0; i < Cin; ++i) {
        float v;
        if (kind == 1) v = src[(size_t)o * 4 * Cin + (size_t)i * 4 + dy * 2 + dx];
        else v = src[(((size_t)o * Cin + i) * KS + dy) * KS + dx];
        packed[((size_t)t * CoutPad + no) * Cin + i] = v;
      }
    }
  }
  if (to_bf16) {
    packed_out.resize(n * 2);
    uint16_t* h = reinterpret_cast<uint16_t*>(packed_out.data());
    for (size_t i = 0; i < n; ++i) h[i] = f32_to_bf16_host(packed[i]);
  } else {
    packed_out.resize(n * 4);
    std::memcpy(packed_out.data(), packed.data(), n * 4);
  }
}

namespace {

// Batch row i of a launch is pass i / nt.  null_mask bit p: pass p reads the null row (class guidance 0b010, joint guidance
// 0b100, otherwise 0); every other pass reads the label row.
__global__ void fill_rows_kernel(int* rows, int n, int nt, int null_mask, int v_label, int v_null) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) rows[i] = ((null_mask >> (i / nt)) & 1) ? v_null : v_label;
}
// Per-image labels: batch row i of a launch is pass i / nt of tile first + i % nt.  The tile's image (third int of its
// tile-list record, the index TileBatch addresses ImageDesc with) selects the image's label slot; a pass whose bit of
// null_mask is set takes null_row, every other pass the image's own label row.  base: row offset of the evaluation inside a step.
__global__ void fill_rows_labels_kernel(int* rows, int n, int nt, const int* tile_yx, int first, const int* slots, int base,
                                        int null_mask, int null_row) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int pass = i / nt, image = tile_yx[3 * (first + (i - pass * nt)) + 2];
  rows[i] = base + (((null_mask >> pass) & 1) ? null_row : slots[image]);
}
__global__ void set_step_kernel(int* step, int v) { *step = v; }
__global__ void rows_api_kernel(int* rows, int n, int odd) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) rows[i] = 2 * i + odd;
}
__global__ void rows_api_labels_kernel(int* rows, int n, int stride, const int* slots) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) rows[i] = stride * i + slots[i];
}


struct HostTensor {
  std::string name;
  std::vector<int64_t> shape;
  std::vector<float> data;
  bool loaded = false;
  size_t numel() const {
    size_t n = 1;
    for (auto s : shape) n *= (size_t)s;
    return n;
  }
};

enum ConvKind { CK_NORMAL = 0, CK_UNSHUFFLE = 1, CK_SHUFFLE = 2 };
struct ConvW {
  int Cin = 0, Cout = 0, CoutPad = 0, KS = 1, stride = 1, pad = 0, mode = CONV_PLAIN, kind = CK_NORMAL;
  int wi = -1, bi = -1;       // indices of the host tensors
  void* w = nullptr;
  void* w3 = nullptr;         // conv3x3_bf16 fast-path packing (bf16 mode, eligible channel counts)
  void* w1 = nullptr;         // conv1x1_bf16 packing (bf16 mode: 1x1 / pixel-shuffle / space-to-depth layers)
  void* wq = nullptr;         // conv3x3_mxfp8 packing (fp8 mode: e4m3 weights + E8M0 block scales)
  void* wq1 = nullptr;        // conv1x1_mxfp8 packing (fp8 mode: the pointwise layers whose inputs have MX-fp8 twins)
  void* ws3 = nullptr;        // conv3x3_split packing (f16x3 mode: (hi, lo) f16 tiles of the scaled weights)
  void* wm3 = nullptr;        // conv3x3_mx2 packing (f16mx2 prototype mode: f16 hi tile + MX-e4m3 planes of w_hi and w_lo)
  void* ws = nullptr;         // conv_igemm_split packing (f16x3 mode: every other layer with Cin % 32 == 0)
  void* ws1 = nullptr;        // conv1x1_split packing (f16x3 mode: 1x1 / pixel-shuffle / space-to-depth layers with Cout % 128 == 0)
  float ws_inv = 1.f;         // 1 / the layer's power-of-two weight scale (f16x3 mode)
  float* bias = nullptr;
};
struct Lin {
  int in_f = 0, out_f = 0, wi = -1, bi = -1;
  float* w = nullptr;
  float* b = nullptr;
};
struct ResW {
  int Cin = 0, Cout = 0, ss_offset = 0;
  ConvW c1, c2, res;
  bool has_res = false;
  int g1i = -1, b1i = -1, g2i = -1, b2i = -1;
  float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr;
  Lin mlp;
};
struct AttnW {
  bool full = false;
  int C = 0;
  int ngi = -1, ogi = -1;
  float *norm_g = nullptr, *out_g = nullptr;
  ConvW qkv, out;
  // f16x3 mode: to_qkv for conv1x1_split with the pre-norm's gain * sqrt(C) folded into the weights (the kernel supplies the
  // per-pixel 1 / ||x||), and the post-norm's gain * sqrt(C) for the RMSNorm tail of to_out (C == 128 sites)
  void* qkv_ws1n = nullptr; float qkv_wsn_inv = 1.f;
  float* out_gs = nullptr;
  // fused LinearAttention block operands (bf16, C = 128 / 256): see linattn_fused.hip, linattn_fused256.hip
  void *f_wkv = nullptr, *f_wq = nullptr, *f_wout = nullptr;
  float* f_g2 = nullptr;
};
struct StageW {
  ResW rb[2];
  AttnW attn;
  ConvW resample;
};

struct Pool {
  struct Buf { void* p; size_t cap; bool busy; };
  std::vector<Buf> bufs;
  // fp8 mode: MX-fp8 twin (e4m3 bytes, E8M0 scales; both pool buffers) of a bf16 activation buffer, made the first time a
  // 3x3 convolution consumes the tensor and reused by later consumers (block inputs feed a second conv as skip connections);
  // released together with the bf16 buffer
  std::map<const void*, std::pair<void*, void*>> twins;
  int64_t total = 0;
  bool no_alloc = false;
  void* get(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    int best = -1;
    for (int i = 0; i < (int)bufs.size(); ++i)
      if (!bufs[i].busy && bufs[i].cap >= bytes && (best < 0 || bufs[i].cap < bufs[best].cap)) best = i;
    if (best >= 0) {
      bufs[best].busy = true;
      return bufs[best].p;
    }
    void* p = nullptr;
    if (no_alloc) {
      set_error("activation pool: allocation requested while a hipGraph is being captured (pool not warm)");
      return nullptr;
    }
    if (hipMalloc(&p, bytes) != hipSuccess) {
      set_error("activation pool: hipMalloc of " + std::to_string(bytes) + " bytes failed");
      return nullptr;
    }
    total += (int64_t)bytes;
    bufs.push_back({p, bytes, true});
    return p;
  }
  void put(void* p) {
    auto t = twins.find(p);
    if (t != twins.end()) {
      const std::pair<void*, void*> qs = t->second;
      twins.erase(t);
      put(qs.first);
      put(qs.second);
    }
    for (auto& b : bufs)
      if (b.p == p) { b.busy = false; return; }
  }
  // Buffers are only ever held within one C-ABI call; an entry point that failed half-way (SRGD_TRY returns) leaves some
  // marked busy, so every entry point starts from a clean slate instead of leaking them forever.
  void reset_busy() {
    for (auto& b : bufs) b.busy = false;
    twins.clear();
  }
  void release_all() {
    for (auto& b : bufs) hipFree(b.p);
    bufs.clear();
    twins.clear();
    total = 0;
  }
};

struct CondTable {
  float* table = nullptr;   // [rows][ss_stride]
  int rows_cap = 0;          // time values the buffers hold ...
  int labels_cap = 0;        // ... at this many label rows per time value (+ the null row)
  float *ls = nullptr, *feat = nullptr, *h1 = nullptr, *t1 = nullptr, *trows = nullptr, *c1 = nullptr, *c2 = nullptr;
};

struct ProfRec { int kc; hipEvent_t a, b; };

const char* kFamilyNames[KC_COUNT] = {"conv_igemm", "conv3x3_bf16", "conv1x1_bf16", "init_conv7x7", "groupnorm_silu", "rmsnorm", "linear_attention",
                                      "full_attention", "final_conv_ddpm_step", "canvas_rng", "conditioning", "conv3x3_mxfp8",
                                      "quantize_mxfp8", "conv1x1_mxfp8", "conv3x3_split", "conv_igemm_split", "conv1x1_split"};

}  // namespace
}  // namespace srgd

using namespace srgd;

struct srgd_engine {
  srgd_unet_config cfg;
  bool bf16 = false;
  int es = 4;
  int dim = 0, time_dim = 0, hid = 0, n_stages = 0;
  std::vector<int> dims;
  std::vector<HostTensor> wt;
  std::map<std::string, int> widx;
  bool finalized = false;
  std::vector<void*> weight_allocs;
  int64_t weight_bytes = 0;

  void* init7_w = nullptr;      // 7x1 x 64-virtual-channel packing of init_conv for the MFMA route
  int init7_coutpad = 0;
  void* init7_w1 = nullptr;     // same weights in the conv1x1_bf16 tile order
  void* init7_ws1 = nullptr;    // f16x3 mode: the same weights split into (hi, lo) f16 tiles for conv1x1_split
  float init7_ws_inv = 1.f;
  float *init_b = nullptr, *final_w = nullptr, *final_b = nullptr, *sin_w = nullptr, *cls_emb = nullptr;
  int init_wi = -1, init_bi = -1, final_wi = -1, final_bi = -1, sin_wi = -1, cls_emb_i = -1;
  Lin time1, time3, cls1, cls3;
  std::vector<StageW> downs, ups;
  ResW mid1, mid2, final_rb;
  AttnW mid_attn;
  std::vector<ResW*> all_rb;
  int ss_stride = 0;
  int stats_slots = 0;          // slots per (sample, group) the last conv wrote into gn_partial
  bool force_generic_conv = false;
  bool force_unfused_attn = false;
  // conv3x3_bf16 can apply the producer's GroupNorm+SiLU while staging its input (GNIN): the separate gn_apply pass over that
  // tensor (2 B read + 2 B written per element) disappears, the MFMA-bound convolution pays ~13 VALU cycles per staged element.
  // Round 3, on the spill-free K loop (profiles/r3/gnin_ab.txt, same box): on for the layers with ONE 128-channel output tile
  // (+1.7 % HR tiles/s: GroupNorm share 10.1 -> 5.9 %, conv3x3 1304 -> 1249 TFLOP/s), off above (the transform is repeated per
  // n-tile: two tiles +1.3 %, all layers -0.7 %).  SRGD_GN_FUSION=0 switches it off, SRGD_GN_FUSION_NTILES=n moves the limit.
  // Round 4, on the cheaper transform (profiles/r4/gnin_ab.txt): one tile / two tiles / all layers / off = 1.3278 / 1.3268 / 1.3106 /
  // 1.2931 HR tiles/s, and with gn_apply's hoisted coefficient loads 1.3657 / 1.3677 and 1.3660 / 1.3676 on a faster box: two
  // tiles is ahead by 0.1 % and takes the GroupNorm share from 6.0 to 5.0 % (one HBM pass less over every 256-channel tensor),
  // so the limit is two now.
  bool mx2 = false;           // SRGD_PRECISION_F16MX2 (prototype): split mode whose 3x3 convolutions run conv3x3_mx2.hip
  bool mx2_pack = true;       // (while packing) this block's 3x3 convolutions take the two-MFMA arithmetic; false: they stay on conv3x3_split
  // blocks nearest the output / input kept on the three-MFMA arithmetic (SRGD_MX2_EXACT_TAIL / _HEAD override).  Default: everything at
  // the tile's own resolution - final block + last up stage (tail 2), first down stage (head 1) - because that is where the error is
  // made (tools/mx2_tail_study.py, profiles/r6/conv3x3_mx2_prototype.txt: configs[1] after 2 steps 2.3e-3 -> 2.3e-4 for 4 % of speed)
  int mx2_exact_tail = 2, mx2_exact_head = 1;
  bool x1 = false;            // SRGD_PRECISION_F16X1: split mode whose halo-kernel 3x3 convolutions contract the hi halves alone (one f16 MFMA per product)
  bool split = false;         // SRGD_PRECISION_F16X3: fp32 tensors, convolutions as three f16 MFMAs per product (conv3x3_split.hip)
  bool fp8 = false;           // SRGD_PRECISION_FP8: 3x3 convolutions on the block-scaled MX-fp8 matrix cores, the rest as bf16
  bool w8 = false;            // SRGD_PRECISION_BF16_W8: conv weights rounded through fp8 e4m3 (per-output-channel scale)
  bool no_gn_fusion = false;
  int split_gn_fusion_max_ntiles = 64;  // f16x3 mode: three MFMAs per staged product make the transform relatively cheaper (SRGD_GN_FUSION_NTILES overrides)
  int gn_fusion_max_ntiles = 2;         // GNIN only where Cout / 128 <= this (the transform is repeated once per n-tile); round 4: 2 (was 1)
  bool no_final_fusion = false;   // SRGD_FINAL_FUSION=0: the last ResnetBlock stores its output and final_step applies the 1x1 (A/B switch)
  bool no_la256 = false;      // SRGD_LA256=0: the C = 256 LinearAttention sites run the unfused chain (A/B switch)
  bool no_rms_fusion = false; // SRGD_RMS_FUSION=0: f16x3 mode runs the RMSNorms around the attention projections as separate passes (A/B switch)
  bool no_conv1x1 = false;    // SRGD_CONV1X1=0: route the pointwise layers through the generic implicit GEMM (A/B switch)
  // fp8 modes: pointwise layers with twinned inputs on the MX matrix cores (conv1x1_mxfp8, 128-pixel tiles: two workgroups
  // per CU).  Per shape +20-40 % over conv1x1_bf16; end to end it only paid once the shared epilogue loaded its tail operand up
  // front: configs[4] 0.430 -> 0.444 HR tiles/s, same box (profiles/r3/mx1x1_ab.txt), for -0.5 dB (fp8) / -1.2 dB
  // (fp8_mixed) against the reference.  SRGD_MX1X1=0 keeps them on conv1x1_bf16.
  bool no_mx1x1 = false;
  bool no_attn_w8 = false;    // SRGD_FP8_ATTN_W=0: fp8 modes keep the attention projections' weights in bf16 (A/B switch)
  unsigned attn_bf16_zones = 1;   // zones whose attention weights stay bf16 on top of fp8_bf16_zones: the first down stage's 256x256 LinearAttention
                                  // site (round 5, tools/fp8_attn_site_study.py); SRGD_FP8_ATTN_BF16_ZONES=<mask> overrides
  int attn_w8_tensors = 0;    // attention weight tensors carried as MX-fp8 (weight-only) after srgd_finalize_weights
  int attn_w8_skipped = 0;    // ... and attention weight tensors left in bf16 because Cin % 32 != 0 (dim-16 test models)
  int mx1x1_min_cin = 0;      // SRGD_MX1X1_MIN_CIN: pointwise layers with fewer input channels stay on conv1x1_bf16
  unsigned fp8_bf16_zones = 0;   // SRGD_FP8_BF16_ZONES (bit mask over Ctx::zone): zones whose 3x3 convs stay bf16 in fp8 mode (study knob)
  bool no_twin_fusion = false;   // SRGD_Q_FUSED=0: fp8 mode quantises every conv input in a separate pass (A/B + bit-equality test)

  Pool pool;
  float* gn_partial = nullptr; size_t gn_partial_cap = 0;
  float *coefA = nullptr, *coefB = nullptr; size_t coef_cap = 0;
  float* la_ws = nullptr; size_t la_ws_cap = 0;
  int* d_rows = nullptr; size_t rows_cap = 0;
  CondTable ct_sampler, ct_api;

  // sampler run state
  srgd_sampler_geometry geo{};
  int *d_tiles_even = nullptr, *d_tiles_odd = nullptr; size_t tiles_cap_even = 0, tiles_cap_odd = 0;
  StepScalars* d_sc = nullptr; int sc_cap = 0;
  int n_steps = 0, run_class = -1;
  bool run_active = false;
  // per-image labels (srgd_sampler_image_labels): the run's K distinct labels own rows 0..K-1 of every time value's K + 1
  // conditioning rows (row K: no label); d_slots[image] is the image's row.  K = 1 without the call: rows (label | none).
  int n_labels = 1;
  bool run_labels = false, run_stepped = false;
  std::vector<float> run_times;           // the run's "time" inputs, kept to rebuild the table for other labels
  int* d_slots = nullptr; size_t slots_cap = 0;
  int* d_slots_api = nullptr; size_t slots_api_cap = 0;   // srgd_unet_forward_labels: label row of each sample
  std::vector<int> slots_host, slots_api_host;            // sources of the uploads (alive until the next one)
  float* rng_tiles = nullptr; size_t rng_tiles_cap = 0;
  EdmScalars* d_edm = nullptr; int edm_cap = 0; bool run_is_edm = false;
  float* rng_canvas = nullptr; size_t rng_canvas_cap = 0;
  // per-image records of the run (kernels.hpp ImageDesc): a same-sized run holds n_images records of one geometry, a mixed run
  // (srgd_sampler_begin_images) one record per image; every canvas kernel and the DDPM step address through them
  std::vector<ImageDesc> images;
  ImageDesc* d_images = nullptr; size_t images_cap = 0;
  bool run_mixed = false;
  int n_grid[2] = {0, 0};                 // tiles of the even / odd grid over all images
  int max_local[2] = {0, 0};              // most tiles of one image per grid (device tile noise: one draw serves every image)
  long max_canvas = 0, max_image = 0;     // largest 3*Hp*Wp / 3*H*W of one image
  struct NoiseClass { int Hp, Wp; long long cnoise_off; };
  std::vector<NoiseClass> classes;        // in order of first appearance; canvas noise of class k at cnoise_off
  size_t class_canvas_elems = 0;          // sum of the classes' 3*Hp*Wp
  std::vector<int> class_n[2];            // tiles of one image of class k in the even / odd grid
  // per-class noise seeds (srgd_sampler_noise_seeds): every device draw is then one batched launch over the classes' streams;
  // d_streams holds three tables of n_classes records: even-step tiles | odd-step tiles | canvas (ring, q_start)
  bool run_seeded = false;
  PhiloxStream* d_streams = nullptr; size_t streams_cap = 0;
  std::vector<PhiloxStream> streams_host;
  size_t stream_max_n[3] = {0, 0, 0};     // largest stream of each table, elements
  int class_tiles[2] = {0, 0};            // sum of class_n: tiles of a seeded step's concatenated draw

  // device-side step counter + per-run hipGraph cache: a DDPM step is one graph per (grid parity, guidance mode);
  // step-dependent values (conditioning row, schedule scalars, RNG stream) are read through d_step, so one captured
  // graph serves every step of that parity.
  int* d_step = nullptr;
  hipStream_t cap_stream = nullptr;
  bool use_graphs = true;
  struct StepKey {                   // everything a captured step bakes in besides what it reads through d_step
    int mode;                        // 0: DDPM step, 1: EDM step
    int parity, passes, kind, sub_batch; float scale; const void *img, *cond, *xs; uint64_t seed; bool last;
    float scale2;                    // joint guidance: the class scale (0 otherwise)
    int tile_first, tile_count; bool ring;
    const void* work;                // EDM step: its scratch canvases
    bool operator==(const StepKey& o) const {
      return mode == o.mode && parity == o.parity && passes == o.passes && kind == o.kind && sub_batch == o.sub_batch &&
             scale == o.scale && scale2 == o.scale2 && img == o.img && cond == o.cond && xs == o.xs && seed == o.seed && last == o.last &&
             tile_first == o.tile_first && tile_count == o.tile_count && ring == o.ring && work == o.work;
    }
  };
  struct StepGraph { StepKey key; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; };   // no exec yet: seen once, run eagerly
  std::vector<StepGraph> graphs;

  // profiling
  bool prof_on = false;
  std::vector<ProfRec> prof;
  std::vector<hipEvent_t> ev_free;
  double fam_flops[KC_COUNT] = {};   // algorithmic FLOPs issued per family while profiling (conv families only)
  double fam_bytes[KC_COUNT] = {};   // algorithmic HBM bytes (operands read once + results written once) per family while profiling

  int reg(const std::string& name, std::vector<int64_t> shape) {
    HostTensor t;
    t.name = name;
    t.shape = std::move(shape);
    wt.push_back(std::move(t));
    widx[name] = (int)wt.size() - 1;
    return (int)wt.size() - 1;
  }
};

static void drop_step_graphs(srgd_engine* e);

namespace {

struct Prof {
  srgd_engine* e; int kc; hipStream_t st; hipEvent_t a{}, b{};
  Prof(srgd_engine* e_, int kc_, hipStream_t st_) : e(e_), kc(kc_), st(st_) {
    if (!e->prof_on) return;
    for (hipEvent_t* ev : {&a, &b}) {
      if (!e->ev_free.empty()) { *ev = e->ev_free.back(); e->ev_free.pop_back(); }
      else hipEventCreate(ev);
    }
    hipEventRecord(a, st);
  }
  ~Prof() {
    if (!e->prof_on) return;
    hipEventRecord(b, st);
    e->prof.push_back({kc, a, b});
  }
};

// ----------------------------------------------------------------------- topology
void reg_conv(srgd_engine* e, ConvW& c, const std::string& wname, const std::string& bname, int Cin, int Cout, int KS,
              int stride, int pad, int kind) {
  c.Cin = Cin; c.Cout = Cout; c.KS = KS; c.stride = stride; c.pad = pad; c.kind = kind;
  c.CoutPad = cdiv(Cout, conv_tile_n()) * conv_tile_n();
  c.mode = (kind == CK_SHUFFLE) ? CONV_PIXEL_SHUFFLE_SILU : CONV_PLAIN;
  if (kind == CK_UNSHUFFLE) c.wi = e->reg(wname, {Cout, 4 * Cin, 1, 1});
  else c.wi = e->reg(wname, {Cout, Cin, kind == CK_SHUFFLE ? 1 : KS, kind == CK_SHUFFLE ? 1 : KS});
  c.bi = bname.empty() ? -1 : e->reg(bname, {Cout});
}

void reg_res(srgd_engine* e, ResW& r, const std::string& p, int Cin, int Cout, int& ss_off) {
  r.Cin = Cin; r.Cout = Cout;
  r.mlp.in_f = e->time_dim; r.mlp.out_f = 2 * Cout;
  r.mlp.wi = e->reg(p + ".mlp.1.weight", {2 * Cout, e->time_dim});
  r.mlp.bi = e->reg(p + ".mlp.1.bias", {2 * Cout});
  reg_conv(e, r.c1, p + ".block1.proj.weight", p + ".block1.proj.bias", Cin, Cout, 3, 1, 1, CK_NORMAL);
  r.g1i = e->reg(p + ".block1.norm.weight", {Cout});
  r.b1i = e->reg(p + ".block1.norm.bias", {Cout});
  reg_conv(e, r.c2, p + ".block2.proj.weight", p + ".block2.proj.bias", Cout, Cout, 3, 1, 1, CK_NORMAL);
  r.g2i = e->reg(p + ".block2.norm.weight", {Cout});
  r.b2i = e->reg(p + ".block2.norm.bias", {Cout});
  r.has_res = Cin != Cout;
  if (r.has_res) reg_conv(e, r.res, p + ".res_conv.weight", p + ".res_conv.bias", Cin, Cout, 1, 1, 0, CK_NORMAL);
  r.ss_offset = ss_off;
  ss_off += 2 * Cout;
  e->all_rb.push_back(&r);
}

void reg_attn(srgd_engine* e, AttnW& a, const std::string& p, int C, bool full) {
  a.full = full; a.C = C;
  a.ngi = e->reg(p + ".norm.g", {1, C, 1, 1});
  reg_conv(e, a.qkv, p + ".to_qkv.weight", "", C, 3 * e->hid, 1, 1, 0, CK_NORMAL);
  if (full) {
    reg_conv(e, a.out, p + ".to_out.weight", p + ".to_out.bias", e->hid, C, 1, 1, 0, CK_NORMAL);
  } else {
    reg_conv(e, a.out, p + ".to_out.0.weight", p + ".to_out.0.bias", e->hid, C, 1, 1, 0, CK_NORMAL);
    a.ogi = e->reg(p + ".to_out.1.g", {1, C, 1, 1});
  }
}

int build_topology(srgd_engine* e) {
  const srgd_unet_config& c = e->cfg;
  if (c.n_stages < 1 || c.n_stages > SRGD_MAX_STAGES) SRGD_FAIL("n_stages out of range");
  if (c.channels != 3) SRGD_FAIL("only channels=3 (6-channel noisy|condition input) is supported");
  if (c.dim_head != 32) SRGD_FAIL("only attn_dim_head=32 is supported");
  if (c.heads < 1 || 256 % c.heads != 0) SRGD_FAIL("attn_heads must divide 256");
  if (c.sinus_dim < 2 || c.sinus_dim % 2) SRGD_FAIL("learned_sinusoidal_dim must be even");
  if (c.dim % 16 != 0) SRGD_FAIL("unet_dim must be a multiple of 16");
  if (c.groups < 1 || c.dim % c.groups != 0) SRGD_FAIL("unet_dim must be divisible by resnet_block_groups");
  if (c.precision < SRGD_PRECISION_FP32 || c.precision > SRGD_PRECISION_F16X1) SRGD_FAIL("unknown precision mode");
  e->mx2 = c.precision == SRGD_PRECISION_F16MX2;
  e->x1 = c.precision == SRGD_PRECISION_F16X1;
  e->split = c.precision == SRGD_PRECISION_F16X3 || e->mx2 || e->x1;
  e->bf16 = c.precision != SRGD_PRECISION_FP32 && !e->split;
  e->w8 = c.precision == SRGD_PRECISION_BF16_W8;
  e->fp8 = c.precision == SRGD_PRECISION_FP8 || c.precision == SRGD_PRECISION_FP8_MIXED;
  // mixed mode: the zones at the tile's own resolution (Ctx::zone 0, 2n, 2n+1) stay on the bf16 3x3 kernel - their
  // activations carry the finest detail and cost 19 dB of the fp8 mode's error (tools/fp8_zone_study.py)
  if (c.precision == SRGD_PRECISION_FP8_MIXED) e->fp8_bf16_zones = 1u | (1u << (2 * c.n_stages)) | (1u << (2 * c.n_stages + 1));
  e->es = e->bf16 ? 2 : 4;
  e->dim = c.dim; e->time_dim = 4 * c.dim; e->hid = c.heads * c.dim_head; e->n_stages = c.n_stages;
  e->dims.push_back(c.dim);
  for (int s = 0; s < c.n_stages; ++s) e->dims.push_back(c.dim * c.dim_mults[s]);
  for (int d : e->dims) {
    if ((d / c.groups) > conv_tile_n() || conv_tile_n() % (d / c.groups) != 0)
      SRGD_FAIL("channels per GroupNorm group must divide 128");
  }
  const int n = c.n_stages, td = e->time_dim;
  e->init_wi = e->reg("init_conv.weight", {c.dim, 6, 7, 7});
  e->init_bi = e->reg("init_conv.bias", {c.dim});
  e->sin_wi = e->reg("time_mlp.0.weights", {c.sinus_dim / 2});
  e->time1 = Lin{c.sinus_dim + 1, td, e->reg("time_mlp.1.weight", {td, c.sinus_dim + 1}), e->reg("time_mlp.1.bias", {td})};
  e->time3 = Lin{td, td, e->reg("time_mlp.3.weight", {td, td}), e->reg("time_mlp.3.bias", {td})};
  if (c.num_classes > 0) {
    e->cls_emb_i = e->reg("class_mlp.0.weight", {c.num_classes, c.dim});
    e->cls1 = Lin{c.dim, td, e->reg("class_mlp.1.weight", {td, c.dim}), e->reg("class_mlp.1.bias", {td})};
    e->cls3 = Lin{td, td, e->reg("class_mlp.3.weight", {td, td}), e->reg("class_mlp.3.bias", {td})};
  }
  int ss = 0;
  e->downs.resize(n);
  e->ups.resize(n);
  for (int s = 0; s < n; ++s) {
    const int din = e->dims[s], dout = e->dims[s + 1];
    const std::string p = "downs." + std::to_string(s);
    reg_res(e, e->downs[s].rb[0], p + ".0", din, din, ss);
    reg_res(e, e->downs[s].rb[1], p + ".1", din, din, ss);
    reg_attn(e, e->downs[s].attn, p + ".2", din, c.full_attn[s] != 0);
    if (s < n - 1) reg_conv(e, e->downs[s].resample, p + ".3.1.weight", p + ".3.1.bias", din, dout, 2, 2, 0, CK_UNSHUFFLE);
    else reg_conv(e, e->downs[s].resample, p + ".3.weight", p + ".3.bias", din, dout, 3, 1, 1, CK_NORMAL);
  }
  const int mid = e->dims[n];
  reg_res(e, e->mid1, "mid_block1", mid, mid, ss);
  reg_attn(e, e->mid_attn, "mid_attn", mid, true);
  reg_res(e, e->mid2, "mid_block2", mid, mid, ss);
  for (int u = 0; u < n; ++u) {
    const int s = n - 1 - u, din = e->dims[s], dout = e->dims[s + 1];
    const std::string p = "ups." + std::to_string(u);
    reg_res(e, e->ups[u].rb[0], p + ".0", dout + din, dout, ss);
    reg_res(e, e->ups[u].rb[1], p + ".1", dout + din, dout, ss);
    reg_attn(e, e->ups[u].attn, p + ".2", dout, c.full_attn[s] != 0);
    if (u < n - 1) reg_conv(e, e->ups[u].resample, p + ".3.net.0.weight", p + ".3.net.0.bias", dout, 4 * din, 1, 1, 0, CK_SHUFFLE);
    else reg_conv(e, e->ups[u].resample, p + ".3.weight", p + ".3.bias", dout, din, 3, 1, 1, CK_NORMAL);
  }
  reg_res(e, e->final_rb, "final_res_block", 2 * c.dim, c.dim, ss);
  e->final_wi = e->reg("final_conv.weight", {3, c.dim, 1, 1});
  e->final_bi = e->reg("final_conv.bias", {3});
  e->ss_stride = ss;
  return 0;
}

// ----------------------------------------------------------------------- weight packing
int upload(srgd_engine* e, const void* host, size_t bytes, void** dev) {
  SRGD_HIP(hipMalloc(dev, bytes));
  e->weight_allocs.push_back(*dev);
  e->weight_bytes += (int64_t)bytes;
  SRGD_HIP(hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
  return 0;
}
int upload_f32(srgd_engine* e, int idx, float** dev) {
  return upload(e, e->wt[idx].data.data(), e->wt[idx].numel() * sizeof(float), (void**)dev);
}

int pack_conv(srgd_engine* e, ConvW& c) {
  std::vector<unsigned char> packed;
  std::vector<float> bias;
  const float* hb = c.bi >= 0 ? e->wt[c.bi].data.data() : nullptr;
  pack_conv_weights(e->wt[c.wi].data.data(), hb, c.kind, c.Cin, c.Cout, c.CoutPad, c.KS, e->bf16, packed, bias);
  SRGD_TRY(upload(e, packed.data(), packed.size(), &c.w));
  if (hb) SRGD_TRY(upload(e, bias.data(), bias.size() * 4, (void**)&c.bias));
  if (e->bf16 && c.kind == CK_NORMAL && c.KS == 3 && c.Cin % 32 == 0 && c.Cout % 128 == 0) {
    std::vector<unsigned short> p3;
    pack_conv3x3_bf16(e->wt[c.wi].data.data(), c.Cin, c.Cout, p3, f32_to_bf16_host);
    SRGD_TRY(upload(e, p3.data(), p3.size() * 2, &c.w3));
  }
  if (e->split && c.Cin % 32 == 0) {
    // f16x3 mode: one power-of-two scale per layer, (hi, lo) f16 halves of the scaled weights in both kernels' layouts
    const float scale = split_weight_scale(e->wt[c.wi].data.data(), e->wt[c.wi].numel(), true);
    c.ws_inv = 1.0f / scale;
    std::vector<unsigned short> ps;
    if (c.kind == CK_NORMAL && c.KS == 3 && c.Cout % 128 == 0 && e->mx2 && e->mx2_pack) {
      std::vector<unsigned char> pm;
      pack_conv3x3_mx2(e->wt[c.wi].data.data(), c.Cin, c.Cout, scale, pm);
      SRGD_TRY(upload(e, pm.data(), pm.size(), &c.wm3));
    } else if (c.kind == CK_NORMAL && c.KS == 3 && c.Cout % 128 == 0) {
      pack_conv3x3_split(e->wt[c.wi].data.data(), c.Cin, c.Cout, true, scale, ps);
      SRGD_TRY(upload(e, ps.data(), ps.size() * 2, &c.ws3));
    }
    pack_conv_weights_split(reinterpret_cast<const float*>(packed.data()), c.KS * c.KS, c.Cin, c.CoutPad, true, scale, ps);
    SRGD_TRY(upload(e, ps.data(), ps.size() * 2, &c.ws));
    if ((c.KS == 1 || c.kind == CK_UNSHUFFLE) && c.Cout % 128 == 0 && c.CoutPad == c.Cout) {
      pack_conv1x1_split(reinterpret_cast<const float*>(packed.data()), c.KS * c.KS, c.Cin, c.Cout, scale, ps);
      SRGD_TRY(upload(e, ps.data(), ps.size() * 2, &c.ws1));
    }
  }
  if (e->fp8 && c.kind == CK_NORMAL && c.KS == 3 && c.Cin % 128 == 0 && c.Cout % 128 == 0) {
    std::vector<unsigned char> pq;
    pack_conv3x3_mxfp8(e->wt[c.wi].data.data(), c.Cin, c.Cout, pq);
    SRGD_TRY(upload(e, pq.data(), pq.size(), &c.wq));
  }
  if (e->bf16 && (c.KS == 1 || c.kind == CK_UNSHUFFLE) && c.Cin % 32 == 0 && c.Cout % 128 == 0 && c.CoutPad == c.Cout) {
    std::vector<unsigned char> f32p;
    std::vector<float> unused;
    pack_conv_weights(e->wt[c.wi].data.data(), hb, c.kind, c.Cin, c.Cout, c.CoutPad, c.KS, false, f32p, unused);
    std::vector<unsigned short> p1;
    pack_conv1x1_bf16(reinterpret_cast<const float*>(f32p.data()), c.KS * c.KS, c.Cin, c.Cout, p1, f32_to_bf16_host);
    SRGD_TRY(upload(e, p1.data(), p1.size() * 2, &c.w1));
    if (e->fp8 && !e->no_mx1x1 && c.Cin % 128 == 0) {
      std::vector<unsigned char> pq1;
      pack_conv1x1_mxfp8(reinterpret_cast<const float*>(f32p.data()), c.KS * c.KS, c.Cin, c.Cout, pq1);
      SRGD_TRY(upload(e, pq1.data(), pq1.size(), &c.wq1));
    }
  }
  return 0;
}

int pack_lin(srgd_engine* e, Lin& l) {
  SRGD_TRY(upload_f32(e, l.wi, &l.w));
  SRGD_TRY(upload_f32(e, l.bi, &l.b));
  return 0;
}
int pack_res(srgd_engine* e, ResW& r) {
  SRGD_TRY(pack_conv(e, r.c1));
  SRGD_TRY(pack_conv(e, r.c2));
  if (r.has_res) SRGD_TRY(pack_conv(e, r.res));
  SRGD_TRY(upload_f32(e, r.g1i, &r.g1));
  SRGD_TRY(upload_f32(e, r.b1i, &r.b1));
  SRGD_TRY(upload_f32(e, r.g2i, &r.g2));
  SRGD_TRY(upload_f32(e, r.b2i, &r.b2));
  SRGD_TRY(pack_lin(e, r.mlp));
  return 0;
}
int pack_attn(srgd_engine* e, AttnW& a) {
  SRGD_TRY(upload_f32(e, a.ngi, &a.norm_g));
  if (a.ogi >= 0) SRGD_TRY(upload_f32(e, a.ogi, &a.out_g));
  SRGD_TRY(pack_conv(e, a.qkv));
  SRGD_TRY(pack_conv(e, a.out));
  if (e->split && a.C % 32 == 0 && a.qkv.Cout % 128 == 0 && a.qkv.CoutPad == a.qkv.Cout) {
    // to_qkv(RMSNorm(x)) = (1 / ||x||) * (W diag(g sqrt(C))) x : fold the gain into the weights, [1][Cout][Cin] order
    const float* w = e->wt[a.qkv.wi].data.data();
    const float* g = e->wt[a.ngi].data.data();
    std::vector<float> wf((size_t)a.qkv.Cout * a.C);
    const float rc = sqrtf((float)a.C);
    for (int o = 0; o < a.qkv.Cout; ++o)
      for (int c = 0; c < a.C; ++c) wf[(size_t)o * a.C + c] = w[(size_t)o * a.C + c] * g[c] * rc;
    const float scale = split_weight_scale(wf.data(), wf.size(), true);
    a.qkv_wsn_inv = 1.0f / scale;
    std::vector<unsigned short> ps;
    pack_conv1x1_split(wf.data(), 1, a.C, a.qkv.Cout, scale, ps);
    SRGD_TRY(upload(e, ps.data(), ps.size() * 2, &a.qkv_ws1n));
    if (a.ogi >= 0) {
      std::vector<float> g2(a.C);
      for (int c = 0; c < a.C; ++c) g2[c] = e->wt[a.ogi].data[c] * rc;
      SRGD_TRY(upload(e, g2.data(), g2.size() * 4, (void**)&a.out_gs));
    }
  }
  if (!a.full && e->bf16 && (a.C == 128 || (a.C == 256 && !e->no_la256)) && e->cfg.heads == 4 && e->cfg.dim_head == 32) {
    std::vector<unsigned short> wkv, wq, wo;
    linattn_fused_pack(e->wt[a.qkv.wi].data.data(), e->wt[a.ngi].data.data(), e->wt[a.out.wi].data.data(), a.C, wkv, wq, wo);
    SRGD_TRY(upload(e, wkv.data(), wkv.size() * 2, &a.f_wkv));
    SRGD_TRY(upload(e, wq.data(), wq.size() * 2, &a.f_wq));
    SRGD_TRY(upload(e, wo.data(), wo.size() * 2, &a.f_wout));
    std::vector<float> g2(a.C);
    for (int c = 0; c < a.C; ++c) g2[c] = e->wt[a.ogi].data[c] * sqrtf((float)a.C);
    SRGD_TRY(upload(e, g2.data(), g2.size() * 4, (void**)&a.f_g2));
  }
  return 0;
}

// Grow-only scratch.  Captured step graphs bake device pointers in: whenever a buffer actually moves, every cached graph
// is dropped (it would otherwise replay onto freed memory, e.g. passes 1 -> 2 -> 1 with device noise, or a larger
// srgd_unet_forward between two steps of a run).
template <typename T> int ensure(srgd_engine* e, T** p, size_t* cap, size_t need_elems) {
  if (*cap >= need_elems) return 0;
  drop_step_graphs(e);
  if (*p) hipFree(*p);
  *p = nullptr;
  SRGD_HIP(hipMalloc((void**)p, need_elems * sizeof(T)));
  *cap = need_elems;
  return 0;
}

// The per-step scalar records of a run (StepScalars into d_sc, EdmScalars into d_edm; the C ABI's host struct has Rec's
// layout).  Unlike ensure() it drops no step graph: the begin entry it serves does that (sampler_begin_common).
template <typename Rec> int upload_step_scalars(srgd_engine* e, Rec** dev, int* cap, int n_steps, const void* host, hipStream_t st) {
  SRGD_HIP(hipSetDevice(e->cfg.device));
  if (*cap < n_steps) {
    if (*dev) hipFree(*dev);
    *dev = nullptr;
    SRGD_HIP(hipMalloc((void**)dev, (size_t)n_steps * sizeof(Rec)));
    *cap = n_steps;
  }
  SRGD_HIP(hipMemcpyAsync(*dev, host, (size_t)n_steps * sizeof(Rec), hipMemcpyHostToDevice, st));
  return 0;
}

// ----------------------------------------------------------------------- forward pieces
struct Ctx {
  srgd_engine* e;
  int nb, H, W;              // batch entries and current resolution
  const int* rows;           // conditioning row of each entry
  const float* table;        // conditioning table in use
  hipStream_t st;
  const int* step_ptr = nullptr;   // sampler: device step counter (row += *step_ptr * step_mul)
  int step_mul = 2;                // conditioning rows per step: 2 (DDPM: label / no label), 4 (EDM: x {sigma_hat, sigma_next})
  int zone = 0;                    // U-Net zone being evaluated: 0..n-1 down stages, n middle, n+1..2n up stages, 2n+1 final block
  // Sampler steps: a [nb*H*W][4] fp32 buffer the last ResnetBlock's epilogue may fill with the 1x1 output convolution of its
  // result (ConvArgs::eps4) instead of storing the block output; eps4_done tells the caller whether that happened.
  float* eps4 = nullptr;
  bool eps4_done = false;
};

// The last ResnetBlock can emit the 1x1 output convolution of its result (16 B of eps per pixel) from its res_conv epilogue only
// on the bf16 streaming-GEMM route at dim 128; everywhere else (fp32 mode, other widths, the A/B switches) the eps4 scratch
// (nb * 256^2 * 16 B: 131 MB at 125 tiles) is not taken from the pool at all.
bool final_fusion_possible(const srgd_engine* e) {
  return e->bf16 && !e->no_final_fusion && !e->no_conv1x1 && !e->force_generic_conv && e->dim == 128 && e->final_rb.has_res &&
         e->final_rb.res.w1 != nullptr;
}

// gn_in: the input is a raw conv output whose GroupNorm+SiLU (coefA/coefB) the fast 3x3 kernel applies while
// staging; *gn_in_done tells the caller whether that happened (otherwise it must run gn_apply first).
bool conv_can_fuse_gn_in(srgd_engine* e, const ConvW& c, int nb, int H, int W) {
  if (e->split) {       // f16x3 mode: conv3x3_split applies it to the fp32 halo pieces in registers, ahead of the split
    if ((!c.ws3 && !c.wm3) || e->force_generic_conv || e->no_gn_fusion || c.Cout / 128 > e->split_gn_fusion_max_ntiles) return false;
    ConvArgs a{};
    a.C0 = c.Cin; a.C1 = 0; a.ps0 = c.Cin; a.B = nb; a.Hin = H; a.Win = W; a.Hout = H; a.Wout = W;
    a.KH = a.KW = c.KS; a.stride = c.stride; a.pad = c.pad; a.Cout = c.Cout; a.CoutPad = c.CoutPad; a.mode = c.mode;
    a.groups = e->cfg.groups; a.gn_partial = e->gn_partial;
    return conv3x3_split_eligible(a);
  }
  if (!e->bf16 || !c.w3 || e->force_generic_conv || e->no_gn_fusion) return false;
  if (c.Cout / 128 > e->gn_fusion_max_ntiles) return false;
  ConvArgs a{};
  a.C0 = c.Cin; a.C1 = 0; a.ps0 = c.Cin; a.B = nb; a.Hin = H; a.Win = W; a.Hout = H; a.Wout = W;
  a.KH = a.KW = c.KS; a.stride = c.stride; a.pad = c.pad; a.Cout = c.Cout; a.CoutPad = c.CoutPad; a.mode = c.mode;
  a.groups = e->cfg.groups; a.gn_partial = e->gn_partial;
  return conv3x3_bf16_eligible(a);
}

struct QTensor { void* q = nullptr; void* s = nullptr; };      // pool buffers: e4m3 [npix][C], E8M0 [npix][C/32]

// fp8 mode: the producer of a tensor that a 3x3 convolution will read writes its MX-fp8 twin in the same epilogue (1 extra
// byte per element) instead of a separate quantisation pass (2 B read + 1 B written); the twin is registered with the pool
// under the bf16 buffer's address and found by q_twin().  A producer without the fused epilogue simply registers nothing.
bool twin_wanted(const srgd_engine* e, bool want, int C) { return e->fp8 && want && !e->no_twin_fusion && C % 128 == 0; }
int twin_alloc(srgd_engine* e, size_t npix, int C, QTensor* t) {
  t->q = e->pool.get(npix * C);
  t->s = e->pool.get(npix * (C / 32));
  return (t->q && t->s) ? 0 : -1;
}
void twin_register(srgd_engine* e, const void* bf16_buf, const QTensor& t) { e->pool.twins[bf16_buf] = {t.q, t.s}; }

int q_twin(Ctx& x, const void* src, int C, int hw, QTensor* t);

// mx_in (fp8 modes): the caller states that the inputs of this pointwise layer are tensors a 3x3 convolution of an fp8 zone
// reads as well, i.e. tensors that have (or, with SRGD_Q_FUSED=0, get on first use) an MX-fp8 twin - the layer may then run on
// the MX matrix cores (conv1x1_mxfp8).  The routing depends on this static statement only, never on whether a twin happens to
// exist yet, so the fused-twin and the separate-quantisation builds take the same path (bit-identical, tested).
int run_conv(Ctx& x, const ConvW& c, const void* in0, int C0, const void* in1, int C1, int Hin, int Win, void* out,
             const void* residual, bool stats, bool gn_in = false, const void* gn_res_src = nullptr, bool want_twin = false,
             float* eps4 = nullptr, bool mx_in = false) {
  srgd_engine* e = x.e;
  ConvArgs a;
  a.in0 = in0; a.in1 = in1; a.C0 = C0; a.C1 = C1; a.ps0 = C0; a.ps1 = C1;
  a.B = x.nb; a.Hin = Hin; a.Win = Win;
  a.Hout = (Hin + 2 * c.pad - c.KS) / c.stride + 1;
  a.Wout = (Win + 2 * c.pad - c.KS) / c.stride + 1;
  a.KH = c.KS; a.KW = c.KS; a.stride = c.stride; a.pad = c.pad;
  a.w = c.w; a.bias = c.bias; a.Cout = c.Cout; a.CoutPad = c.CoutPad;
  a.out = out; a.residual = residual; a.mode = c.mode;
  a.gn_partial = stats ? e->gn_partial : nullptr;
  a.groups = e->cfg.groups;
  a.gn_res_src = gn_res_src; a.gn_res_a = gn_res_src ? e->coefA : nullptr; a.gn_res_b = gn_res_src ? e->coefB : nullptr;
  if (C0 + C1 != c.Cin) SRGD_FAIL("internal: conv input channel mismatch");
  const bool fast = e->bf16 && c.w3 && !e->force_generic_conv && conv3x3_bf16_eligible(a);
  const bool fast1 = !fast && e->bf16 && c.w1 && !e->force_generic_conv && !e->no_conv1x1 && !stats && conv1x1_bf16_eligible(a);
  if (eps4 && fast1 && !e->no_final_fusion && gn_res_src && c.Cout == 128 && !twin_wanted(e, want_twin, c.Cout)) {
    a.eps4 = eps4; a.fin_w = e->final_w; a.fin_b = e->final_b;
    if (conv1x1_bf16_eligible(a)) x.eps4_done = true;
    else a.eps4 = nullptr;
  }
  // fp8 modes: a pointwise layer of an fp8 zone whose inputs are twinned tensors runs on the MX matrix cores (conv1x1_mxfp8)
  const bool fastq1 = fast1 && mx_in && e->fp8 && c.wq1 && !e->no_mx1x1 && c.KS * c.KS * c.Cin >= e->mx1x1_min_cin &&
                      !((e->fp8_bf16_zones >> x.zone) & 1u) && conv1x1_mxfp8_eligible(a);
  QTensor mq0, mq1;
  if (fastq1) {                                   // (a twin that does not exist yet is quantised here, as for the 3x3 convolutions)
    SRGD_TRY(q_twin(x, in0, C0, Hin * Win, &mq0));
    if (in1) SRGD_TRY(q_twin(x, in1, C1, Hin * Win, &mq1));
  }
  const bool split3 = e->split && (c.ws3 || c.wm3) && !e->force_generic_conv && conv3x3_split_eligible(a);
  const bool split1 = e->split && !split3 && c.ws1 && !stats && !e->force_generic_conv && !e->no_conv1x1 && conv1x1_split_eligible(a);
  const bool splitg = e->split && !split3 && !split1 && c.ws && conv_igemm_split_eligible(a);
  const int fam = split3 ? KC_CONV3S : split1 ? KC_CONV1S : splitg ? KC_CONVS : fast ? KC_CONV3 : fastq1 ? KC_CONV1Q : fast1 ? KC_CONV1 : KC_CONV;
  Prof p(e, fam, x.st);
  if (e->prof_on) {
    e->fam_flops[fam] += 2.0 * (double)x.nb * a.Hout * a.Wout * c.Cout * (double)(c.KS * c.KS * c.Cin);
    // algorithmic bytes: every input pixel row once, the weights once, the result once (+ the in-place GroupNorm2 tail operand,
    // the residual, the MX-fp8 twin); with the fused output convolution 16 B of eps per pixel replace the result row
    const double npi = (double)x.nb * Hin * Win, npo = (double)x.nb * a.Hout * a.Wout;
    const double in_es = fastq1 ? 1.0 + 1.0 / 32 : (double)e->es;       // MX route: 1 B per element + 1 scale byte per 32
    double by = npi * c.Cin * in_es + (double)c.KS * c.KS * c.Cin * c.Cout * in_es;
    by += a.eps4 ? npo * 16.0 : npo * c.Cout * e->es;
    if (gn_res_src) by += npo * c.Cout * e->es;
    if (residual) by += npo * c.Cout * e->es;
    if (fast1 && twin_wanted(e, want_twin, c.mode == CONV_PIXEL_SHUFFLE_SILU ? c.Cout / 4 : c.Cout)) by += npo * c.Cout * (1.0 + 1.0 / 32);
    e->fam_bytes[fam] += by;
  }
  if (fast1) {
    const bool ps = c.mode == CONV_PIXEL_SHUFFLE_SILU;
    const int Cq = ps ? c.Cout / 4 : c.Cout;
    QTensor tw;
    if (twin_wanted(e, want_twin, Cq)) {
      SRGD_TRY(twin_alloc(e, (size_t)x.nb * a.Hout * a.Wout * (ps ? 4 : 1), Cq, &tw));
      a.out_q = tw.q; a.out_s = tw.s;
    }
    if (fastq1) SRGD_TRY(conv1x1_mxfp8(a, mq0.q, mq0.s, mq1.q, mq1.s, c.wq1, x.st));
    else SRGD_TRY(conv1x1_bf16(a, c.w1, x.st));
    if (tw.q) twin_register(e, out, tw);
    return 0;
  }
  if (fast) {
    if (stats) e->stats_slots = conv3x3_bf16_stats_slots(a);
    return conv3x3_bf16(a, c.w3, gn_in ? e->coefA : nullptr, gn_in ? e->coefB : nullptr, x.st);
  }
  if (split3) {
    if (stats) e->stats_slots = conv3x3_bf16_stats_slots(a);
    if (c.wm3) return conv3x3_mx2(a, c.wm3, c.ws_inv, x.st, gn_in ? e->coefA : nullptr, gn_in ? e->coefB : nullptr);
    return conv3x3_split(a, c.ws3, c.ws_inv, true, x.st, gn_in ? e->coefA : nullptr, gn_in ? e->coefB : nullptr, 0, e->x1 ? 1 : 3);
  }
  if (gn_in) SRGD_FAIL("internal: fused input GroupNorm requested on the generic conv path");
  if (split1) return conv1x1_split(a, c.ws1, c.ws_inv, x.st);
  if (stats) e->stats_slots = cdiv(a.Hout * a.Wout, conv_tile_m());
  if (splitg) return conv_igemm_split(a, c.ws, c.ws_inv, true, x.st);
  return conv_igemm(a, e->bf16, x.st);
}

// ---- MX-fp8 route of the 3x3 convolutions (fp8 mode) ---------------------------------------------------------------

ConvArgs conv3_args(Ctx& x, const ConvW& c, int C0, int C1, int H, int W, void* out, bool stats) {
  srgd_engine* e = x.e;
  ConvArgs a{};
  a.C0 = C0; a.C1 = C1; a.ps0 = C0; a.ps1 = C1; a.B = x.nb; a.Hin = H; a.Win = W; a.Hout = H; a.Wout = W;
  a.KH = a.KW = c.KS; a.stride = c.stride; a.pad = c.pad; a.bias = c.bias; a.Cout = c.Cout; a.CoutPad = c.CoutPad;
  a.out = out; a.mode = c.mode; a.gn_partial = stats ? e->gn_partial : nullptr; a.groups = e->cfg.groups;
  return a;
}
bool conv_is_q(Ctx& x, const ConvW& c, int C0, int C1, int H, int W, bool stats) {
  srgd_engine* e = x.e;
  if (!e->fp8 || !c.wq || e->force_generic_conv) return false;
  if ((e->fp8_bf16_zones >> x.zone) & 1u) return false;            // this zone's 3x3 convolutions stay on the bf16 kernel
  return conv3x3_mxfp8_eligible(conv3_args(x, c, C0, C1, H, W, nullptr, stats));
}
int q_alloc(Ctx& x, int C, int hw, QTensor* t) {
  const size_t npix = (size_t)x.nb * hw;
  t->q = x.e->pool.get(npix * C);
  t->s = x.e->pool.get(npix * (C / 32));
  return (t->q && t->s) ? 0 : -1;
}
void q_free(Ctx& x, QTensor& t) {
  if (t.q) x.e->pool.put(t.q);
  if (t.s) x.e->pool.put(t.s);
  t = QTensor{};
}
// the MX-fp8 twin of a bf16 pool tensor: quantised on first use, found again afterwards, freed with the tensor (Pool::put)
int q_twin(Ctx& x, const void* src, int C, int hw, QTensor* t) {
  Pool& pool = x.e->pool;
  auto it = pool.twins.find(src);
  if (it != pool.twins.end()) {
    t->q = it->second.first; t->s = it->second.second;
    return 0;
  }
  SRGD_TRY(q_alloc(x, C, hw, t));
  pool.twins[src] = {t->q, t->s};
  Prof p(x.e, KC_QUANT, x.st);
  if (x.e->prof_on) x.e->fam_bytes[KC_QUANT] += (double)x.nb * hw * C * (2.0 + 1.0 + 1.0 / 32);
  return quant_mxfp8(src, t->q, t->s, (long)x.nb * hw, C, x.st);
}
int run_conv_q(Ctx& x, const ConvW& c, const QTensor& in0, int C0, const QTensor& in1, int C1, int H, int W, void* out,
               bool stats, bool want_twin = false) {
  srgd_engine* e = x.e;
  ConvArgs a = conv3_args(x, c, C0, C1, H, W, out, stats);
  if (C0 + C1 != c.Cin) SRGD_FAIL("internal: conv input channel mismatch");
  QTensor tw;
  if (twin_wanted(e, want_twin, c.Cout)) {
    SRGD_TRY(twin_alloc(e, (size_t)x.nb * H * W, c.Cout, &tw));
    a.out_q = tw.q; a.out_s = tw.s;
  }
  Prof p(e, KC_CONVQ, x.st);
  if (e->prof_on) {
    e->fam_flops[KC_CONVQ] += 2.0 * (double)x.nb * H * W * c.Cout * (double)(9 * c.Cin);
    const double np = (double)x.nb * H * W;
    e->fam_bytes[KC_CONVQ] += np * c.Cin * (1.0 + 1.0 / 32) + 9.0 * c.Cin * c.Cout * (1.0 + 1.0 / 32) + np * c.Cout * 2.0 +
                              (tw.q ? np * c.Cout * (1.0 + 1.0 / 32) : 0.0);
  }
  if (stats) e->stats_slots = conv3x3_mxfp8_stats_slots(a);
  SRGD_TRY(conv3x3_mxfp8(a, in0.q, in0.s, in1.q, in1.s, c.wq, x.st));
  if (tw.q) twin_register(e, out, tw);
  return 0;
}
// a 3x3 convolution of bf16 pool tensors through the fp8 route, on their MX-fp8 twins
int run_conv_q_from_bf16(Ctx& x, const ConvW& c, const void* in0, int C0, const void* in1, int C1, int H, int W, void* out,
                         bool stats, bool want_twin = false) {
  QTensor a, b;
  SRGD_TRY(q_twin(x, in0, C0, H * W, &a));
  if (C1) SRGD_TRY(q_twin(x, in1, C1, H * W, &b));
  return run_conv_q(x, c, a, C0, b, C1, H, W, out, stats, want_twin);
}

int run_gn(Ctx& x, const float* gamma, const float* beta, int C, int hw, int ss_offset /* <0: none */, void* buf,
           const void* residual, bool finalize_only = false, bool want_twin = false) {
  srgd_engine* e = x.e;
  Prof p(e, KC_GN, x.st);
  GnFinalizeArgs f;
  f.partial = e->gn_partial; f.nslots = e->stats_slots; f.B = x.nb; f.C = C; f.groups = e->cfg.groups; f.hw = hw;
  f.gamma = gamma; f.beta = beta;
  f.ss_table = ss_offset >= 0 ? x.table : nullptr; f.ss_rows = x.rows; f.step_ptr = x.step_ptr; f.step_mul = x.step_mul;
  f.ss_stride = e->ss_stride; f.ss_offset = ss_offset < 0 ? 0 : ss_offset; f.eps = 1e-5f;
  f.coefA = e->coefA; f.coefB = e->coefB;
  f.x = buf; f.x_is_bf16 = e->bf16;                // buf holds the producing convolution's output until gn_apply / the consumer runs
  SRGD_TRY(gn_finalize(f, x.st));
  if (finalize_only) return 0;                     // the consumer conv applies y = silu(A x + B) while staging
  QTensor tw;
  if (twin_wanted(e, want_twin, C)) SRGD_TRY(twin_alloc(e, (size_t)x.nb * hw, C, &tw));
  if (e->prof_on)      // one read + one write of the tensor (+ the identity residual, + the MX-fp8 twin)
    e->fam_bytes[KC_GN] += (double)x.nb * hw * C * (e->es * (residual ? 3.0 : 2.0) + (tw.q ? 1.0 + 1.0 / 32 : 0.0));
  SRGD_TRY(gn_apply_silu(buf, buf, residual, e->coefA, e->coefB, x.nb, hw, C, e->bf16, x.st, tw.q, tw.s));
  if (tw.q) twin_register(e, buf, tw);
  return 0;
}

// f16x3 mode: can this res_conv run on conv1x1_split with the GroupNorm2 + SiLU + residual tail in its epilogue?
bool split_gntail_possible(const Ctx& x, const ConvW& c, int C0, int C1) {
  const srgd_engine* e = x.e;
  if (!c.ws1 || e->force_generic_conv || e->no_conv1x1) return false;
  ConvArgs a{};
  a.C0 = C0; a.C1 = C1; a.ps0 = C0; a.ps1 = C1; a.in1 = C1 ? (const void*)1 : nullptr; a.B = x.nb; a.Hin = x.H; a.Win = x.W; a.Hout = x.H; a.Wout = x.W;
  a.KH = a.KW = 1; a.stride = 1; a.pad = 0; a.Cout = c.Cout; a.CoutPad = c.CoutPad; a.mode = CONV_PLAIN;
  a.gn_res_src = (const void*)1; a.gn_res_a = (const float*)1; a.gn_res_b = (const float*)1;
  return conv1x1_split_eligible(a);
}

// ResnetBlock (model.py:261-285); returns a pool buffer [nb,H,W,Cout]
int res_block(Ctx& x, const ResW& r, const void* in0, int C0, const void* in1, int C1, void** out, bool want_twin = false,
              float* eps4 = nullptr) {
  srgd_engine* e = x.e;
  const int hw = x.H * x.W;
  const size_t bytes = (size_t)x.nb * hw * r.Cout * e->es;
  void* u = e->pool.get(bytes);
  void* v = e->pool.get(bytes);
  if (!u || !v) return -1;
  if (conv_is_q(x, r.c1, C0, C1, x.H, x.W, true) && conv_is_q(x, r.c2, r.Cout, 0, x.H, x.W, true)) {
    // fp8 mode: both 3x3 convolutions on the MX matrix cores.  conv1 reads quantised copies of the block input; the
    // GroupNorm1-apply + SiLU pass writes conv2's input directly as MX-fp8 (1 byte per element instead of 2).
    SRGD_TRY(run_conv_q_from_bf16(x, r.c1, in0, C0, in1, C1, x.H, x.W, u, true));
    SRGD_TRY(run_gn(x, r.g1, r.b1, r.Cout, hw, r.ss_offset, u, nullptr, true));
    QTensor qu;
    SRGD_TRY(q_alloc(x, r.Cout, hw, &qu));
    { Prof p(e, KC_GN, x.st);
      if (e->prof_on) e->fam_bytes[KC_GN] += (double)x.nb * hw * r.Cout * (2.0 + 1.0 + 1.0 / 32);
      SRGD_TRY(gn_apply_silu_mxfp8(u, qu.q, qu.s, e->coefA, e->coefB, x.nb, hw, r.Cout, x.st)); }
    SRGD_TRY(run_conv_q(x, r.c2, qu, r.Cout, QTensor{}, 0, x.H, x.W, v, true));
    q_free(x, qu);
  } else {
  SRGD_TRY(run_conv(x, r.c1, in0, C0, in1, C1, x.H, x.W, u, nullptr, true));
  const bool fuse = conv_can_fuse_gn_in(e, r.c2, x.nb, x.H, x.W);
  SRGD_TRY(run_gn(x, r.g1, r.b1, r.Cout, hw, r.ss_offset, u, nullptr, fuse));
  SRGD_TRY(run_conv(x, r.c2, u, r.Cout, nullptr, 0, x.H, x.W, v, nullptr, true, fuse));
  }
  if (r.has_res && e->bf16) {
    // GroupNorm2 + SiLU + (+ res_conv(x)) evaluated in the 1x1 res_conv's epilogue, in place over v
    SRGD_TRY(run_gn(x, r.g2, r.b2, r.Cout, hw, -1, v, nullptr, true));
    SRGD_TRY(run_conv(x, r.res, in0, C0, in1, C1, x.H, x.W, v, nullptr, false, false, v, want_twin, eps4, true));
  } else if (r.has_res && e->split && !e->no_gn_fusion && split_gntail_possible(x, r.res, C0, C1)) {
    // f16x3 mode: the same fusion in conv1x1_split's epilogue (SEPI_GNTAIL)
    SRGD_TRY(run_gn(x, r.g2, r.b2, r.Cout, hw, -1, v, nullptr, true));
    SRGD_TRY(run_conv(x, r.res, in0, C0, in1, C1, x.H, x.W, v, nullptr, false, false, v));
  } else if (r.has_res) {
    SRGD_TRY(run_conv(x, r.res, in0, C0, in1, C1, x.H, x.W, u, nullptr, false));   // u is free again: reuse it
    SRGD_TRY(run_gn(x, r.g2, r.b2, r.Cout, hw, -1, v, u));
  } else {
    if (in1) SRGD_FAIL("internal: identity residual with two sources");
    SRGD_TRY(run_gn(x, r.g2, r.b2, r.Cout, hw, -1, v, in0, false, want_twin));
  }
  e->pool.put(u);
  *out = v;
  return 0;
}

// x + attn(x)  (model.py:703,:709,:718); returns a pool buffer [nb,H,W,C]
int attn_block(Ctx& x, const AttnW& a, const void* in, void** out, bool want_twin = false) {
  srgd_engine* e = x.e;
  const int hw = x.H * x.W;
  const long npix = (long)x.nb * hw;
  if (a.f_wkv && !e->force_unfused_attn && linattn_fused_eligible(a.C, e->cfg.heads, e->cfg.dim_head, hw, e->bf16)) {
    Prof p(e, KC_LINATTN, x.st);
    void* y = e->pool.get((size_t)npix * a.C * e->es);
    if (!y) return -1;
    if (linattn_fused_workspace(x.nb, hw) / sizeof(float) > e->la_ws_cap) SRGD_FAIL("internal: fused attention workspace too small");
    QTensor tw;
    if (twin_wanted(e, want_twin, a.C)) SRGD_TRY(twin_alloc(e, (size_t)npix, a.C, &tw));
    // la1 reads x once, la2 reads x again and writes y: three passes over a C-channel tensor (+ the twin)
    if (e->prof_on) e->fam_bytes[KC_LINATTN] += (double)npix * a.C * (3.0 * e->es + (tw.q ? 1.0 + 1.0 / 32 : 0.0));
    SRGD_TRY(linattn_fused(in, y, x.nb, hw, a.C, a.f_wkv, a.f_wq, a.f_wout, a.out.bias, a.f_g2, e->la_ws, x.st, tw.q, tw.s));
    if (tw.q) twin_register(e, y, tw);
    *out = y;
    return 0;
  }
  void* nrm = e->pool.get((size_t)npix * a.C * e->es);
  void* qkv = e->pool.get((size_t)npix * 3 * e->hid * e->es);
  void* att = e->pool.get((size_t)npix * e->hid * e->es);
  if (!nrm || !qkv || !att) return -1;
  // f16x3 mode: both RMSNorms ride in the projections' kernels where conv1x1_split covers the shape (conv1x1_split.hip: RMS_IN,
  // SEPI_RMS_RESIDUAL); SRGD_RMS_FUSION=0 keeps the separate passes (A/B switch)
  auto split1_args = [&](const ConvW& c, const void* src, int Cin, void* dst) {
    ConvArgs q;
    q.in0 = src; q.in1 = nullptr; q.C0 = Cin; q.C1 = 0; q.ps0 = Cin; q.ps1 = 0;
    q.B = x.nb; q.Hin = x.H; q.Win = x.W; q.Hout = x.H; q.Wout = x.W; q.KH = q.KW = 1; q.stride = 1; q.pad = 0;
    q.w = nullptr; q.bias = c.bias; q.Cout = c.Cout; q.CoutPad = c.CoutPad; q.out = dst; q.residual = nullptr; q.mode = CONV_PLAIN;
    q.gn_partial = nullptr; q.groups = e->cfg.groups; q.gn_res_src = nullptr; q.gn_res_a = q.gn_res_b = nullptr;
    return q;
  };
  bool qkv_done = false;
  if (e->split && a.qkv_ws1n && !e->no_rms_fusion && !e->no_conv1x1 && !e->force_generic_conv) {
    ConvArgs q = split1_args(a.qkv, in, a.C, qkv);
    q.rms_in = true;
    if (conv1x1_split_eligible(q)) {
      Prof p(e, KC_CONV1S, x.st);
      if (e->prof_on) {
        e->fam_flops[KC_CONV1S] += 2.0 * (double)npix * a.qkv.Cout * a.C;
        e->fam_bytes[KC_CONV1S] += (double)npix * (a.C + a.qkv.Cout) * 4.0 + (double)a.C * a.qkv.Cout * 4.0;
      }
      SRGD_TRY(conv1x1_split(q, a.qkv_ws1n, a.qkv_wsn_inv, x.st));
      qkv_done = true;
    }
  }
  if (!qkv_done) {
    { Prof p(e, KC_RMS, x.st);
      if (e->prof_on) e->fam_bytes[KC_RMS] += (double)npix * a.C * e->es * 2.0;
      SRGD_TRY(rms_norm(in, nrm, nullptr, a.norm_g, npix, a.C, e->bf16, x.st)); }
    SRGD_TRY(run_conv(x, a.qkv, nrm, a.C, nullptr, 0, x.H, x.W, qkv, nullptr, false));
  }
  if (a.full) {
    Prof p(e, KC_FULLATTN, x.st);
    if (e->prof_on) e->fam_bytes[KC_FULLATTN] += (double)npix * e->hid * e->es * 4.0;      // q, k, v read, o written
    SRGD_TRY(full_attention(qkv, att, x.nb, hw, e->cfg.heads, e->cfg.dim_head, e->bf16, x.st));
  } else {
    Prof p(e, KC_LINATTN, x.st);
    const size_t need = linear_attention_workspace(x.nb, hw, e->cfg.heads, e->cfg.dim_head) / sizeof(float);
    if (need > e->la_ws_cap) SRGD_FAIL("internal: linear attention workspace too small");
    if (e->prof_on) e->fam_bytes[KC_LINATTN] += (double)npix * e->hid * e->es * 6.0;       // k, v read; q, k-stats read; o written (two passes)
    SRGD_TRY(linear_attention(qkv, att, x.nb, hw, e->cfg.heads, e->cfg.dim_head, e->la_ws, e->bf16, x.st));
  }
  e->pool.put(qkv);
  if (a.full) {
    SRGD_TRY(run_conv(x, a.out, att, e->hid, nullptr, 0, x.H, x.W, nrm, in, false, false, nullptr, want_twin));   // + bias + residual x
  } else {
    bool out_done = false;
    if (e->split && a.out.ws1 && a.out_gs && a.C == 128 && !e->no_rms_fusion && !e->no_conv1x1 && !e->force_generic_conv) {
      ConvArgs q = split1_args(a.out, att, e->hid, nrm);
      q.residual = in; q.rms_out_g = a.out_gs;
      if (conv1x1_split_eligible(q)) {
        Prof p(e, KC_CONV1S, x.st);
        if (e->prof_on) {
          e->fam_flops[KC_CONV1S] += 2.0 * (double)npix * a.C * e->hid;
          e->fam_bytes[KC_CONV1S] += (double)npix * (e->hid + 2.0 * a.C) * 4.0 + (double)a.C * e->hid * 4.0;
        }
        SRGD_TRY(conv1x1_split(q, a.out.ws1, a.out.ws_inv, x.st));
        out_done = true;
      }
    }
    if (!out_done) {
      SRGD_TRY(run_conv(x, a.out, att, e->hid, nullptr, 0, x.H, x.W, nrm, nullptr, false));
      Prof p(e, KC_RMS, x.st);
      if (e->prof_on) e->fam_bytes[KC_RMS] += (double)npix * a.C * e->es * 3.0;
      SRGD_TRY(rms_norm(nrm, nrm, in, a.out_g, npix, a.C, e->bf16, x.st));                     // RMSNorm then + x
    }
  }
  e->pool.put(att);
  *out = nrm;
  return 0;
}

int ensure_scratch(srgd_engine* e, int nb, int H, int W) {
  const int hw = H * W;
  const int cmax = *std::max_element(e->dims.begin(), e->dims.end());
  // GroupNorm partial slots per (sample, group): generic kernel one per 128-pixel tile; the 3x3 fast paths one per contributing
  // wave of a 256-pixel patch (conv3x3_bf16_stats_slots: 4, or 8 per 128-channel tile a group spans)
  const size_t slots = std::max((size_t)cdiv(hw, conv_tile_m()), (size_t)cdiv(hw, 256) * std::max(4, cmax / e->cfg.groups / 16));
  SRGD_TRY(ensure(e, &e->gn_partial, &e->gn_partial_cap, (size_t)nb * e->cfg.groups * slots * 2));
  size_t need = (size_t)nb * cmax;
  if (e->coef_cap < need) {
    drop_step_graphs(e);
    if (e->coefA) hipFree(e->coefA);
    e->coefA = e->coefB = nullptr;
    SRGD_HIP(hipMalloc((void**)&e->coefA, 2 * need * 4));     // one allocation: [scale | shift] (conv3x3 GNIN reads both)
    e->coefB = e->coefA + need;
    e->coef_cap = need;
  }
  SRGD_TRY(ensure(e, &e->la_ws, &e->la_ws_cap,
                  std::max(linear_attention_workspace(nb, hw, e->cfg.heads, e->cfg.dim_head), linattn_fused_workspace(nb, hw)) / 4));
  SRGD_TRY(ensure(e, &e->d_rows, &e->rows_cap, (size_t)nb));
  return 0;
}

// 7x7 input conv on MFMA: `padded` is the gathered [entries][H+6][W+8][8] image (see kernels.hpp)
int run_init7(srgd_engine* e, const void* padded, int entries, int H, int W, void* out, hipStream_t st) {
  ConvArgs a;
  a.in0 = padded; a.in1 = nullptr; a.C0 = 64; a.C1 = 0; a.ps0 = 8; a.ps1 = 0;
  a.B = entries; a.Hin = H + 6; a.Win = W + 8; a.Hout = H; a.Wout = W;
  a.KH = 7; a.KW = 1; a.stride = 1; a.pad = 0;
  a.w = e->init7_w; a.bias = e->init_b; a.Cout = e->dim; a.CoutPad = e->init7_coutpad;
  a.out = out; a.residual = nullptr; a.mode = CONV_PLAIN; a.gn_partial = nullptr; a.groups = e->cfg.groups;
  a.gn_res_src = nullptr; a.gn_res_a = a.gn_res_b = nullptr;
  if (e->split && e->init7_ws1 && !e->no_conv1x1 && !e->force_generic_conv && conv1x1_split_eligible(a))
    return conv1x1_split(a, e->init7_ws1, e->init7_ws_inv, st);
  if (e->bf16 && e->init7_w1 && !e->no_conv1x1 && !e->force_generic_conv && conv1x1_bf16_eligible(a)) {
    QTensor tw;                                    // fp8 mode: x0 feeds the first and the last ResnetBlock's 3x3 convolutions
    const bool x0q = e->fp8 && (!((e->fp8_bf16_zones >> 0) & 1u) || !((e->fp8_bf16_zones >> (2 * e->n_stages + 1)) & 1u));
    if (twin_wanted(e, x0q, e->dim)) {
      SRGD_TRY(twin_alloc(e, (size_t)entries * H * W, e->dim, &tw));
      a.out_q = tw.q; a.out_s = tw.s;
    }
    SRGD_TRY(conv1x1_bf16(a, e->init7_w1, st));
    if (tw.q) twin_register(e, out, tw);
    return 0;
  }
  return conv_igemm(a, e->bf16, st);
}

// fp8 modes: do the 3x3 convolutions of U-Net zone `zone` run on the MX kernel?  A producer writes a tensor's MX-fp8 twin only
// when one of the tensor's consumers does (in fp8_mixed mode the 256x256 zones read bf16: their inputs need no twin)
static bool zone_is_q(const srgd_engine* e, int zone) { return e->fp8 && !((e->fp8_bf16_zones >> zone) & 1u); }

// The U-Net between init_conv and final_conv.  x0: [nb,H,W,dim] (kept alive by the caller).
int unet_body(Ctx& x, void* x0, void** out) {
  srgd_engine* e = x.e;
  const int n = e->n_stages;
  const int f = 1 << (n - 1);
  if (x.H % f || x.W % f) SRGD_FAIL("your input dimensions need to be divisible by " + std::to_string(f) + ", given the unet");
  std::vector<void*> skips;
  void* cur = x0;
  const int H0 = x.H, W0 = x.W;
  for (int s = 0; s < n; ++s) {
    const StageW& sw = e->downs[s];
    const int C = e->dims[s];
    x.zone = s;
    void *a, *b, *c;
    // want_twin flags (fp8 mode only): true where the tensor is read by a 3x3 convolution later - a: next block + skip,
    // c: skip (+ the last stage's 3x3 resampler), d: the next stage's first block
    // consumers: a -> the stage's second block (zone s) and the skip (up-stage zone 2n - s); c -> the skip and, in the last
    // stage, the 3x3 resampler; d -> the next stage (zone s + 1; s + 1 == n: the middle)
    SRGD_TRY(res_block(x, sw.rb[0], cur, C, nullptr, 0, &a, zone_is_q(e, s) || zone_is_q(e, 2 * n - s)));
    if (cur != x0) e->pool.put(cur);
    skips.push_back(a);
    SRGD_TRY(res_block(x, sw.rb[1], a, C, nullptr, 0, &b));
    const bool cq = zone_is_q(e, 2 * n - s) || (s == n - 1 && zone_is_q(e, s));      // c is read by 3x3 convolutions of fp8 zones
    SRGD_TRY(attn_block(x, sw.attn, b, &c, cq));
    e->pool.put(b);
    skips.push_back(c);
    const ConvW& rs = sw.resample;
    const int Ho = (s < n - 1) ? x.H / 2 : x.H, Wo = (s < n - 1) ? x.W / 2 : x.W;
    void* d = e->pool.get((size_t)x.nb * Ho * Wo * rs.Cout * e->es);
    if (!d) return -1;
    const bool dq = zone_is_q(e, s + 1);
    if (conv_is_q(x, rs, C, 0, x.H, x.W, false)) SRGD_TRY(run_conv_q_from_bf16(x, rs, c, C, nullptr, 0, x.H, x.W, d, false, dq));
    else SRGD_TRY(run_conv(x, rs, c, C, nullptr, 0, x.H, x.W, d, nullptr, false, false, nullptr, dq, nullptr, cq));
    x.H = Ho; x.W = Wo;
    cur = d;
  }
  {
    void *a, *b, *c;
    const int C = e->dims[n];
    x.zone = n;
    SRGD_TRY(res_block(x, e->mid1, cur, C, nullptr, 0, &a));
    e->pool.put(cur);
    SRGD_TRY(attn_block(x, e->mid_attn, a, &b, zone_is_q(e, n)));
    e->pool.put(a);
    SRGD_TRY(res_block(x, e->mid2, b, C, nullptr, 0, &c, zone_is_q(e, n + 1)));
    e->pool.put(b);
    cur = c;
  }
  for (int u = 0; u < n; ++u) {
    const StageW& sw = e->ups[u];
    const int s = n - 1 - u, din = e->dims[s], dout = e->dims[s + 1];
    x.zone = n + 1 + u;
    void *a, *b, *c;
    void* sk = skips.back(); skips.pop_back();
    const bool zq = zone_is_q(e, n + 1 + u);
    SRGD_TRY(res_block(x, sw.rb[0], cur, dout, sk, din, &a, zq));
    e->pool.put(cur); e->pool.put(sk);
    sk = skips.back(); skips.pop_back();
    SRGD_TRY(res_block(x, sw.rb[1], a, dout, sk, din, &b));
    e->pool.put(a); e->pool.put(sk);
    // a twin of the attention output: the last stage resamples with a 3x3 convolution; a softmax-attention stage (to_out's
    // epilogue writes the twin for 1 B per element) feeds its K-heavy PixelShuffle 1x1 on the MX matrix cores
    const bool psq = zq && !e->no_mx1x1 && sw.attn.full && sw.resample.wq1 != nullptr;
    SRGD_TRY(attn_block(x, sw.attn, b, &c, (u == n - 1 && zq) || psq));
    e->pool.put(b);
    const ConvW& rs = sw.resample;
    const int Ho = (u < n - 1) ? x.H * 2 : x.H, Wo = (u < n - 1) ? x.W * 2 : x.W;
    void* d = e->pool.get((size_t)x.nb * Ho * Wo * din * e->es);
    if (!d) return -1;
    const bool dq = zone_is_q(e, n + 2 + u);                      // the next up stage, or the final block (zone 2n + 1)
    if (conv_is_q(x, rs, dout, 0, x.H, x.W, false)) SRGD_TRY(run_conv_q_from_bf16(x, rs, c, dout, nullptr, 0, x.H, x.W, d, false, dq));
    else SRGD_TRY(run_conv(x, rs, c, dout, nullptr, 0, x.H, x.W, d, nullptr, false, false, nullptr, dq, nullptr, psq));
    e->pool.put(c);
    x.H = Ho; x.W = Wo;
    cur = d;
  }
  if (x.H != H0 || x.W != W0) SRGD_FAIL("internal: resolution bookkeeping");
  void* fin;
  x.zone = 2 * n + 1;
  x.eps4_done = false;
  SRGD_TRY(res_block(x, e->final_rb, cur, e->dim, x0, e->dim, &fin, false, x.eps4));
  e->pool.put(cur);
  *out = fin;
  return 0;
}

// Conditioning table: K + 1 rows for every log-SNR value i - row i*(K+1) + k carries the class embedding of class_ids[k],
// row i*(K+1) + K none; columns = concatenated per-ResnetBlock (scale | shift) vectors.  K = 1 is the one-label layout
// (rows 2i, 2i+1; class_ids[0] < 0: no label, both rows alike).  Every label's rows come from the launches a run with
// that label alone makes, so they hold the same bits.
int compute_conditioning(srgd_engine* e, CondTable& ct, const float* ls_host, int n, const int* class_ids, int K, hipStream_t st) {
  Prof p(e, KC_COND, st);
  const int td = e->time_dim, half = e->cfg.sinus_dim / 2, nf = e->cfg.sinus_dim + 1;
  if (K < 1) SRGD_FAIL("internal: conditioning table without a label row");
  for (int k = 0; k < K; ++k) {
    if (class_ids[k] >= e->cfg.num_classes) SRGD_FAIL("class label out of range");
    if (class_ids[k] < 0 && K > 1) SRGD_FAIL("class label out of range");
  }
  const int K1 = K + 1;
  if (n > ct.rows_cap || K > ct.labels_cap) {
    const int nc = std::max(n, ct.rows_cap), kc = std::max(K, ct.labels_cap);
    for (float** q : {&ct.table, &ct.ls, &ct.feat, &ct.h1, &ct.t1, &ct.trows, &ct.c1, &ct.c2})
      if (*q) { hipFree(*q); *q = nullptr; }
    ct.rows_cap = ct.labels_cap = 0;
    SRGD_HIP(hipMalloc((void**)&ct.table, (size_t)(kc + 1) * nc * e->ss_stride * 4));
    SRGD_HIP(hipMalloc((void**)&ct.ls, (size_t)nc * 4));
    SRGD_HIP(hipMalloc((void**)&ct.feat, (size_t)nc * nf * 4));
    SRGD_HIP(hipMalloc((void**)&ct.h1, (size_t)nc * td * 4));
    SRGD_HIP(hipMalloc((void**)&ct.trows, (size_t)(kc + 1) * nc * td * 4));
    SRGD_HIP(hipMalloc((void**)&ct.c1, (size_t)td * 4));
    SRGD_HIP(hipMalloc((void**)&ct.c2, (size_t)td * 4));
    ct.rows_cap = nc;
    ct.labels_cap = kc;
  }
  SRGD_HIP(hipMemcpyAsync(ct.ls, ls_host, (size_t)n * 4, hipMemcpyHostToDevice, st));
  SRGD_TRY(time_features(ct.ls, e->sin_w, half, n, ct.feat, st));
  SRGD_TRY(linear_rows(ct.feat, nf, e->time1.w, e->time1.b, ct.h1, td, n, nf, td, ACT_GELU, nullptr, 0, st));
  // rows i*K1 + K: t ; rows i*K1 + k: t + class embedding k
  SRGD_TRY(linear_rows(ct.h1, td, e->time3.w, e->time3.b, ct.trows + (size_t)K * td, K1 * td, n, td, td, ACT_NONE, nullptr, 0, st));
  for (int k = 0; k < K; ++k) {
    float* rows_k = ct.trows + (size_t)k * td;
    if (class_ids[k] >= 0) {
      SRGD_TRY(linear_rows(e->cls_emb + (size_t)class_ids[k] * e->dim, e->dim, e->cls1.w, e->cls1.b, ct.c1, td, 1, e->dim, td,
                           ACT_GELU, nullptr, 0, st));
      SRGD_TRY(linear_rows(ct.c1, td, e->cls3.w, e->cls3.b, ct.c2, td, 1, td, td, ACT_NONE, nullptr, 0, st));
      SRGD_TRY(linear_rows(ct.h1, td, e->time3.w, e->time3.b, rows_k, K1 * td, n, td, td, ACT_NONE, ct.c2, 0, st));
    } else {
      SRGD_TRY(linear_rows(ct.h1, td, e->time3.w, e->time3.b, rows_k, K1 * td, n, td, td, ACT_NONE, nullptr, 0, st));
    }
  }
  for (ResW* r : e->all_rb)
    SRGD_TRY(linear_rows(ct.trows, td, r->mlp.w, r->mlp.b, ct.table + r->ss_offset, e->ss_stride, K1 * n, td, 2 * r->Cout,
                         ACT_SILU_IN, nullptr, 0, st));
  return 0;
}

// The distinct labels of ids[0..n) in order of first appearance, and each entry's index among them
int label_slots(const srgd_engine* e, const int32_t* ids, int n, std::vector<int>& labels, std::vector<int>& slots) {
  labels.clear();
  slots.resize(n);
  for (int i = 0; i < n; ++i) {
    if (ids[i] < 0 || ids[i] >= e->cfg.num_classes) SRGD_FAIL("class label out of range");
    const auto it = std::find(labels.begin(), labels.end(), (int)ids[i]);
    slots[i] = (int)(it - labels.begin());
    if (it == labels.end()) labels.push_back(ids[i]);
  }
  return 0;
}

// Conditioning rows of one U-Net launch of a sampler step: evaluation `ev` of the step (EDM: 0 at sigma_hat, 1 at sigma_next),
// entries [p * nt, (p + 1) * nt) = pass p; null_mask bit p: pass p takes the null row (class guidance: pass 1, joint guidance:
// pass 2).  The step's own rows are added on the device (Ctx::step_mul).
void launch_step_rows(srgd_engine* e, int nb, int nt, const int* tiles, int first, int ev, int null_mask, hipStream_t st) {
  if (e->run_labels) {
    const int K = e->n_labels;
    hipLaunchKernelGGL(fill_rows_labels_kernel, dim3(cdiv(nb, 256)), dim3(256), 0, st, e->d_rows, nb, nt, tiles, first,
                       e->d_slots, ev * (K + 1), null_mask, K);
    return;
  }
  const int row_label = e->run_class >= 0 ? 0 : 1, row_null = 1;
  hipLaunchKernelGGL(fill_rows_kernel, dim3(cdiv(nb, 256)), dim3(256), 0, st, e->d_rows, nb, nt, null_mask, 2 * ev + row_label,
                     2 * ev + row_null);
}

// what a network evaluation of a sampler step needs besides its tiles
struct StepEval {
  int passes, guidance_kind;
  float guidance_scale;
  float *img, *x_start;      // the canvases the final step updates
  int ev;                    // evaluation of the step whose conditioning rows it takes (EDM: 0 at sigma_hat, 1 at sigma_next)
  int evals;                 // evaluations per step the conditioning table holds: 1 (DDPM), 2 (EDM, both solvers)
  float class_scale = 0.f;   // joint guidance (passes 3, kind 3): s_l; guidance_scale is s_c
};

// One U-Net evaluation of one launch's tiles, the same for every sampler step: input conv from the canvases -> conditioning
// rows -> U-Net body -> fused output conv + step update scattered into the canvases.  The two launches that differ between the
// steps come in as callables: gather(use_cond_mask, padded) fills the input conv's haloed image, final_launch(fa) sets the
// FinalStepArgs fields of its own (noise, noise_per_class, sc: zero on arrival) and launches the step's final kernel.
// The order of pool gets / puts and of launches is fixed: it is the topology of a captured step, and under Pool::no_alloc the
// pool's reuse pattern decides the addresses.
template <typename Gather, typename Final>
int eval_tile_batch(srgd_engine* e, const TileBatch& tb, const StepEval& s, hipStream_t st, Gather&& gather, Final&& final_launch) {
  const int tile = tb.tile, nt = tb.ntiles, nb = nt * s.passes;
  // the second pass of a guided step: without the condition (condition guidance, kind 2: mask bit p = pass p sees it) or on
  // the null conditioning row (class guidance, kind 1).  Joint guidance (three passes, kind 3): [0, nt) full, [nt, 2nt) without
  // the condition, [2nt, 3nt) on the null row
  const bool joint = s.passes == 3;
  const int mask = joint ? 0x5 : (s.passes == 2 && s.guidance_kind == 2) ? 0x1 : 0x3;
  const int null_mask = joint ? 0x4 : (s.passes == 2 && s.guidance_kind == 1) ? 0x2 : 0x0;
  void* x0 = e->pool.get((size_t)nb * tile * tile * e->dim * e->es);
  if (!x0) return -1;
  {
    Prof p(e, KC_INIT, st);
    void* padded = e->pool.get((size_t)nb * (tile + 6) * (tile + 8) * 8 * e->es);
    if (!padded) return -1;
    SRGD_TRY(gather(mask, padded));
    SRGD_TRY(run_init7(e, padded, nb, tile, tile, x0, st));
    e->pool.put(padded);
  }
  // conditioning row = base + evals * (K+1) * step (the step's share is added on the device: Ctx::step_mul), base = (K+1) * ev +
  // (label row / K: none); K = 1 unless the run has per-image labels
  launch_step_rows(e, nb, nt, tb.tile_yx, tb.first, s.ev, null_mask, st);
  Ctx x{e, nb, tile, tile, e->d_rows, e->ct_sampler.table, st, e->d_step, s.evals * (e->n_labels + 1)};
  void* act = nullptr;
  float* eps4 = final_fusion_possible(e) ? (float*)e->pool.get((size_t)nb * tile * tile * 16) : nullptr;
  if (final_fusion_possible(e) && !eps4) return -1;
  x.eps4 = eps4;
  SRGD_TRY(unet_body(x, x0, &act));
  FinalStepArgs fa{};
  fa.act = act; fa.C = e->dim; fa.passes = s.passes; fa.guidance = s.guidance_scale; fa.guidance2 = s.class_scale;
  fa.w = e->final_w; fa.bias = e->final_b; fa.img = s.img; fa.x_start = s.x_start;
  fa.step_ptr = e->d_step;
  fa.eps4 = x.eps4_done ? eps4 : nullptr;
  { Prof p(e, KC_FINAL, st); SRGD_TRY(final_launch(fa)); }
  if (eps4) e->pool.put(eps4);
  e->pool.put(act);
  e->pool.put(x0);
  return 0;
}

// what step_prologue works out for a step entry
struct StepPlan {
  int parity;                // grid of the step
  bool last;
  int tile_first, tile_count;   // the (normalised) range of the grid's image-major tile list this call covers
  int sub_batch;             // tiles per U-Net launch
};

// What every step entry does before its launches: the argument checks (messages under the entry's `name`; `null_arg` is the
// entry's test of its own pointers, reported after the step check), the tile range (tile_count < 0: to the end of the grid),
// the size of a launch, and the scratch for it - every allocation of a step happens before any capture.
int step_prologue(srgd_engine* e, const char* name, bool edm, bool null_arg, int step, int tile_first, int tile_count, int passes,
                  int guidance_kind, int sub_batch, StepPlan* plan, bool joint = false) {
  const std::string nm(name);
  if (!e || !e->run_active || e->run_is_edm != edm) SRGD_FAIL(nm + ": call " + (edm ? "srgd_edm_begin" : "srgd_sampler_begin") + " first");
  if (step < 0 || step >= e->n_steps) SRGD_FAIL(nm + ": step out of range");
  if (null_arg) SRGD_FAIL(nm + ": null argument");
  if (joint) {               // the DDPM entry decoded the joint form itself: three passes, kind 3
    if (edm || passes != 3 || guidance_kind != 3) SRGD_FAIL(nm + ": internal: joint form");
  } else {
    if (passes != 1 && passes != 2) SRGD_FAIL(nm + ": passes must be 1 or 2" + (edm ? "" : " (or 3: joint guidance)"));
    if (passes == 2 && guidance_kind != 1 && guidance_kind != 2) SRGD_FAIL(nm + ": guidance_kind must be 1 or 2");
  }
  if (sub_batch < 1) SRGD_FAIL(nm + ": sub_batch must be >= 1");
  SRGD_HIP(hipSetDevice(e->cfg.device));
  const int parity = step & 1;
  const int n = e->n_grid[parity];
  if (tile_count < 0) tile_count = n - tile_first;
  if (tile_first < 0 || tile_count < 0 || tile_first + tile_count > n) SRGD_FAIL(nm + "_tiles: tile range outside the grid");
  e->run_stepped = true;
  // at most the range's tiles per launch (a whole grid is never empty - the begin entries reject one - so for an entry without
  // a range this is min(sub_batch, n))
  sub_batch = std::max(1, std::min(sub_batch, std::max(tile_count, 1)));
  // balanced launches: the same number of U-Net launches, but of (almost) equal size - 1,089 tiles at a limit of 125 run as
  // 9 x 121, not 8 x 125 + 89, and a rank's 137-tile slice of a sharded canvas as 69 + 68, not 125 + 12 (a 12-tile launch
  // fills a fraction of the chip on the deep layers and costs about as much as a 16-tile one).  Tiles are independent within
  // a step, so the result does not depend on how a step's tiles are grouped (tested bit-identical).
  if (tile_count > sub_batch) sub_batch = cdiv(tile_count, cdiv(tile_count, sub_batch));
  e->pool.reset_busy();
  SRGD_TRY(ensure_scratch(e, sub_batch * passes, e->geo.tile, e->geo.tile));
  *plan = StepPlan{parity, step == e->n_steps - 1, tile_first, tile_count, sub_batch};
  return 0;
}

// The last act of a step entry before the step's launches: the step index goes to the device counter they read it through.
// Not part of step_prologue: the entry's own noise-buffer allocations come between the two, ahead of the counter's.
int set_device_step(srgd_engine* e, int step, hipStream_t st) {
  if (!e->d_step) SRGD_HIP(hipMalloc((void**)&e->d_step, sizeof(int)));
  hipLaunchKernelGGL(set_step_kernel, dim3(1), dim3(1), 0, st, e->d_step, step);
  return 0;
}

}  // namespace

// Graph cache shared by the DDPM and the EDM step: the first occurrence of a key runs eagerly (it warms the activation pool and
// every lazily-set kernel attribute), the second is captured on a private stream (the caller's may be the legacy default
// stream, which cannot capture; nothing executes during capture), later ones replay on the caller's stream.
extern "C++" {
template <typename Launch>
static int run_step_through_graph(srgd_engine* e, const srgd_engine::StepKey& key, hipStream_t st, Launch&& launch) {
  srgd_engine::StepGraph* sg = nullptr;
  for (auto& c : e->graphs)
    if (c.key == key) sg = &c;
  if (!sg) {
    e->graphs.push_back({key});
    return launch(st);
  }
  if (!sg->exec) {
    if (!e->cap_stream) SRGD_HIP(hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking));
    SRGD_HIP(hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeThreadLocal));
    e->pool.no_alloc = true;
    const int rc = launch(e->cap_stream);
    e->pool.no_alloc = false;
    hipGraph_t graph = nullptr;
    const hipError_t ce = hipStreamEndCapture(e->cap_stream, &graph);
    if (rc != 0) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (ce != hipSuccess || !graph) SRGD_FAIL(std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
    hipGraphExec_t exec = nullptr;
    const hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (ie != hipSuccess) { (void)hipGraphDestroy(graph); SRGD_FAIL(std::string("hipGraphInstantiate: ") + hipGetErrorString(ie)); }
    sg->graph = graph;
    sg->exec = exec;
  }
  SRGD_HIP(hipGraphLaunch(sg->exec, st));
  return 0;
}
}  // extern "C++"

// ======================================================================= C ABI
extern "C" {

const char* srgd_last_error(void) { return srgd::last_error(); }
const char* srgd_version(void) { return "srgd_hip 0.1 (gfx950)"; }

int srgd_create(const srgd_unet_config* cfg, srgd_engine** out) {
  if (!cfg || !out) SRGD_FAIL("srgd_create: null argument");
  int ndev = 0;
  SRGD_HIP(hipGetDeviceCount(&ndev));
  if (ndev == 0) SRGD_FAIL("srgd_create: no HIP device (this library has no CPU fallback)");
  SRGD_HIP(hipSetDevice(cfg->device));
  std::unique_ptr<srgd_engine> e(new srgd_engine());
  e->cfg = *cfg;
  SRGD_TRY(build_topology(e.get()));
  if (const char* v = getenv("SRGD_GN_FUSION")) e->no_gn_fusion = atoi(v) == 0;   // experiment switch (see no_gn_fusion)
  e->mx2_exact_tail = env_int("SRGD_MX2_EXACT_TAIL", e->mx2_exact_tail);
  e->mx2_exact_head = env_int("SRGD_MX2_EXACT_HEAD", e->mx2_exact_head);
  if (const char* v = getenv("SRGD_GN_FUSION_NTILES")) e->gn_fusion_max_ntiles = e->split_gn_fusion_max_ntiles = atoi(v);
  if (const char* v = getenv("SRGD_GRAPHS")) e->use_graphs = atoi(v) != 0;
  if (const char* v = getenv("SRGD_CONV1X1")) e->no_conv1x1 = atoi(v) == 0;
  if (const char* v = getenv("SRGD_RMS_FUSION")) e->no_rms_fusion = atoi(v) == 0;
  // fp8_mixed is the quality-oriented fp8 mode: its pointwise layers stay on conv1x1_bf16 unless asked for (the MX pointwise
  // kernel buys ~3 % there and costs 1.2 dB against the reference; round-3 advisor finding).  fp8 keeps them on the MX cores.
  e->no_mx1x1 = e->cfg.precision == SRGD_PRECISION_FP8_MIXED;
  if (const char* v = getenv("SRGD_MX1X1")) e->no_mx1x1 = atoi(v) == 0;
  if (const char* v = getenv("SRGD_MX1X1_MIN_CIN")) e->mx1x1_min_cin = atoi(v);
  if (const char* v = getenv("SRGD_FP8_ATTN_W")) e->no_attn_w8 = atoi(v) == 0;
  if (const char* v = getenv("SRGD_FP8_ATTN_BF16_ZONES")) e->attn_bf16_zones = (unsigned)strtoul(v, nullptr, 0);
  if (const char* v = getenv("SRGD_LA256")) e->no_la256 = atoi(v) == 0;
  if (const char* v = getenv("SRGD_FINAL_FUSION")) e->no_final_fusion = atoi(v) == 0;
  if (const char* v = getenv("SRGD_Q_FUSED")) e->no_twin_fusion = atoi(v) == 0;
  if (const char* v = getenv("SRGD_FP8_BF16_ZONES")) e->fp8_bf16_zones = (unsigned)strtoul(v, nullptr, 0);
  *out = e.release();
  return 0;
}

int srgd_destroy(srgd_engine* e) {
  if (!e) return 0;
  hipSetDevice(e->cfg.device);
  hipDeviceSynchronize();
  drop_step_graphs(e);
  if (e->cap_stream) hipStreamDestroy(e->cap_stream);
  if (e->d_step) hipFree(e->d_step);
  for (void* p : e->weight_allocs) hipFree(p);
  e->pool.release_all();
  for (void* p : {(void*)e->gn_partial, (void*)e->coefA, (void*)e->la_ws, (void*)e->d_rows,
                  (void*)e->d_tiles_even, (void*)e->d_tiles_odd, (void*)e->d_sc, (void*)e->d_edm, (void*)e->rng_tiles,
                  (void*)e->rng_canvas, (void*)e->d_images, (void*)e->d_slots, (void*)e->d_slots_api, (void*)e->d_streams})
    if (p) hipFree(p);
  for (CondTable* ct : {&e->ct_sampler, &e->ct_api})
    for (float* q : {ct->table, ct->ls, ct->feat, ct->h1, ct->t1, ct->trows, ct->c1, ct->c2})
      if (q) hipFree(q);
  for (auto& r : e->prof) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
  for (auto ev : e->ev_free) hipEventDestroy(ev);
  delete e;
  return 0;
}

int srgd_num_weights(const srgd_engine* e) { return e ? (int)e->wt.size() : -1; }

int srgd_weight_info(const srgd_engine* e, int index, char* name, size_t name_cap, int64_t shape[4], int* ndim) {
  if (!e || index < 0 || index >= (int)e->wt.size()) SRGD_FAIL("srgd_weight_info: bad index");
  const HostTensor& t = e->wt[index];
  if (name && name_cap) {
    std::strncpy(name, t.name.c_str(), name_cap - 1);
    name[name_cap - 1] = 0;
  }
  if (ndim) *ndim = (int)t.shape.size();
  if (shape) for (size_t i = 0; i < t.shape.size() && i < 4; ++i) shape[i] = t.shape[i];
  return 0;
}

int srgd_load_weight(srgd_engine* e, const char* name, const float* host_data, const int64_t* shape, int ndim) {
  if (!e || !name || !host_data) SRGD_FAIL("srgd_load_weight: null argument");
  if (e->finalized) SRGD_FAIL("srgd_load_weight: weights already finalized");
  std::string key(name);
  if (key.rfind("model.", 0) == 0) key = key.substr(6);
  auto it = e->widx.find(key);
  if (it == e->widx.end()) SRGD_FAIL("Unexpected key(s) in state_dict: \"" + std::string(name) + "\"");
  HostTensor& t = e->wt[it->second];
  bool same = (int)t.shape.size() == ndim;
  for (int i = 0; same && i < ndim; ++i) same = t.shape[i] == shape[i];
  if (!same) SRGD_FAIL("size mismatch for " + key);
  t.data.assign(host_data, host_data + t.numel());
  t.loaded = true;
  return 0;
}

int srgd_finalize_weights(srgd_engine* e) {
  if (!e) SRGD_FAIL("null engine");
  if (e->finalized) return 0;
  std::string missing;
  for (auto& t : e->wt)
    if (!t.loaded) missing += (missing.empty() ? "" : ", ") + t.name;
  if (!missing.empty()) SRGD_FAIL("Missing key(s) in state_dict: " + missing);
  SRGD_HIP(hipSetDevice(e->cfg.device));
  if (e->w8) {
    // every convolution weight [O, I, kh, kw] (RMSNorm gains are [1, C, 1, 1] and stay), one scale per output channel
    for (auto& t : e->wt) {
      if (t.shape.size() != 4 || t.shape[0] <= 1) continue;
      const size_t per = t.numel() / (size_t)t.shape[0];
      for (int64_t o = 0; o < t.shape[0]; ++o) {
        float* w = t.data.data() + (size_t)o * per;
        float amax = 0.f;
        for (size_t i = 0; i < per; ++i) amax = std::max(amax, std::fabs(w[i]));
        if (amax == 0.f) continue;
        const float scale = amax / 448.0f;
        for (size_t i = 0; i < per; ++i) w[i] = round_through_e4m3(w[i] / scale) * scale;
      }
    }
  }
  if (e->fp8 && !e->no_attn_w8) {
    // fp8 modes (BASELINE configs[4]: "fp8 conv + attention weights"): the projections of all attention sites - to_qkv and
    // to_out of LinearAttention / Attention (reference model.py:300-303, 341-342), incl. the ones the fused LinearAttention
    // kernels fold into their register-resident operands - are carried as MX-fp8: e4m3 elements, one E8M0 scale per (output
    // channel, 32 input channels), the engine's scale rule (mx_block_exponent), dequantised here at pack time; the kernels
    // keep multiplying bf16 activations with the (now e4m3-valued) bf16 weights - a weight-FORMAT emulation: numerics of e4m3
    // storage, no speed or memory gain yet.  Exact: an e4m3 value times a power of two is a bf16 value.
    // Placement (round 5, tools/fp8_attn_site_study.py, profiles/r5/fp8_attn_site_study.json; PSNR against the reference on the
    // configs[4] one-tile fixture / at configs[1]'s geometry): bf16 weights at all nine sites 36.5 / 28.0 dB; any ONE site in e4m3
    // 36.3-36.9; all nine 35.1 / 26.8 under either scale rule (E8M0 per 32 input channels or per output channel: 35.09 vs 35.06);
    // all but the first down stage's 256x256 LinearAttention site (zone 0) 36.9 / 27.8.  Shipped: e4m3 at eight of the nine sites
    // in "fp8" (zone 0 keeps bf16 weights; "fp8_mixed" additionally keeps the last up stage's, as its 3x3 convolutions do).
    // SRGD_FP8_ATTN_W=0 keeps all of them in bf16, SRGD_FP8_ATTN_BF16_ZONES=<mask> chooses the zones (A/B switches).
    for (auto& t : e->wt) {
      if (t.shape.size() != 4 || t.shape[2] != 1 || t.shape[3] != 1 || t.shape[0] <= 1) continue;
      if (t.name.find("to_qkv.weight") == std::string::npos && t.name.find("to_out.weight") == std::string::npos &&
          t.name.find("to_out.0.weight") == std::string::npos)
        continue;
      if (t.shape[1] % 32) { e->attn_w8_skipped += 1; continue; }      // no whole 32-channel block: the tensor stays bf16 (counted)
      // zone of the site (Ctx::zone: down stage s -> s, middle -> n, up stage s -> n + 1 + s): the zones that keep bf16 3x3
      // convolutions (fp8_mixed: everything at the tile's own resolution; SRGD_FP8_BF16_ZONES) keep bf16 attention weights too -
      // measured on the configs[4] fixture: e4m3 weights at the two 256x256-resolution LinearAttention sites alone take
      // fp8_mixed from 53.3 dB to 34.8 dB against the reference (the level of bf16_w8, 35.3 dB)
      int zone = e->n_stages;
      if (t.name.rfind("downs.", 0) == 0) zone = atoi(t.name.c_str() + 6);
      else if (t.name.rfind("ups.", 0) == 0) zone = e->n_stages + 1 + atoi(t.name.c_str() + 4);
      if ((e->fp8_bf16_zones | e->attn_bf16_zones) & (1u << zone)) continue;
      const int64_t O = t.shape[0], I = t.shape[1];
      for (int64_t o = 0; o < O; ++o) {
        for (int64_t k0 = 0; k0 < I; k0 += 32) {
          float* w = t.data.data() + (size_t)o * I + k0;
          float amax = 0.f;
          for (int k = 0; k < 32; ++k) amax = std::max(amax, std::fabs(w[k]));
          const int ex = mx_block_exponent(amax);
          const float inv = std::ldexp(1.0f, -ex), sc = std::ldexp(1.0f, ex);
          for (int k = 0; k < 32; ++k) w[k] = round_through_e4m3(w[k] * inv) * sc;
        }
      }
      e->attn_w8_tensors += 1;
    }
    if (e->attn_w8_skipped)          // (dim-16 test models: to_qkv has 16 input channels) - said once per engine, not silently
      fprintf(stderr, "[srgd] fp8 mode: %d attention weight tensor(s) carried as MX-e4m3, %d left in bf16 (input channels not a multiple of 32)\n",
              e->attn_w8_tensors, e->attn_w8_skipped);
  }
  // 7x7 input conv: OIHW [dim,6,7,7] -> 7 taps (dy) x 64 virtual channels (dx*8 + ci), see kernels.hpp
  {
    const std::vector<float>& s = e->wt[e->init_wi].data;
    SRGD_TRY(upload_f32(e, e->init_bi, &e->init_b));
    // MFMA route: [dy][CoutPad][dx*8 + ci] (dx = 7 and ci = 6,7 stay zero)
    e->init7_coutpad = cdiv(e->dim, conv_tile_n()) * conv_tile_n();
    std::vector<float> q((size_t)7 * e->init7_coutpad * 64, 0.f);
    for (int o = 0; o < e->dim; ++o)
      for (int ci = 0; ci < 6; ++ci)
        for (int dy = 0; dy < 7; ++dy)
          for (int dx = 0; dx < 7; ++dx)
            q[((size_t)dy * e->init7_coutpad + o) * 64 + dx * 8 + ci] = s[(((size_t)o * 6 + ci) * 7 + dy) * 7 + dx];
    if (e->bf16) {
      std::vector<unsigned short> h(q.size());
      for (size_t i = 0; i < q.size(); ++i) h[i] = f32_to_bf16_host(q[i]);
      SRGD_TRY(upload(e, h.data(), h.size() * 2, &e->init7_w));
      if (e->init7_coutpad == e->dim) {          // streaming-GEMM route (conv1x1_bf16.hip, 7x1 gather)
        std::vector<unsigned short> p1;
        pack_conv1x1_bf16(q.data(), 7, 64, e->dim, p1, f32_to_bf16_host);
        SRGD_TRY(upload(e, p1.data(), p1.size() * 2, &e->init7_w1));
      }
    } else {
      SRGD_TRY(upload(e, q.data(), q.size() * 4, &e->init7_w));
      if (e->split && e->init7_coutpad == e->dim) {
        const float scale = split_weight_scale(q.data(), q.size(), true);
        e->init7_ws_inv = 1.0f / scale;
        std::vector<unsigned short> ps;
        pack_conv1x1_split(q.data(), 7, 64, e->dim, scale, ps);
        SRGD_TRY(upload(e, ps.data(), ps.size() * 2, &e->init7_ws1));
      }
    }
  }
  SRGD_TRY(upload_f32(e, e->final_wi, &e->final_w));
  SRGD_TRY(upload_f32(e, e->final_bi, &e->final_b));
  SRGD_TRY(upload_f32(e, e->sin_wi, &e->sin_w));
  SRGD_TRY(pack_lin(e, e->time1));
  SRGD_TRY(pack_lin(e, e->time3));
  if (e->cfg.num_classes > 0) {
    SRGD_TRY(upload_f32(e, e->cls_emb_i, &e->cls_emb));
    SRGD_TRY(pack_lin(e, e->cls1));
    SRGD_TRY(pack_lin(e, e->cls3));
  }
  // f16mx2 prototype: the blocks nearest the output (final block = 1, + last up stage = 2, ...) / the input (first down stage = 1, ...)
  // can stay on the three-MFMA arithmetic - an error made there reaches x_start undamped
  const int n_st = (int)e->downs.size();
  for (int i = 0; i < n_st; ++i) {
    auto& s = e->downs[i];
    e->mx2_pack = i >= e->mx2_exact_head;
    SRGD_TRY(pack_res(e, s.rb[0])); SRGD_TRY(pack_res(e, s.rb[1]));
    SRGD_TRY(pack_attn(e, s.attn)); SRGD_TRY(pack_conv(e, s.resample));
  }
  e->mx2_pack = true;
  SRGD_TRY(pack_res(e, e->mid1)); SRGD_TRY(pack_attn(e, e->mid_attn)); SRGD_TRY(pack_res(e, e->mid2));
  for (int i = 0; i < n_st; ++i) {
    auto& s = e->ups[i];
    e->mx2_pack = (n_st - 1 - i) + 2 > e->mx2_exact_tail;      // last up stage = tail level 2
    SRGD_TRY(pack_res(e, s.rb[0])); SRGD_TRY(pack_res(e, s.rb[1]));
    SRGD_TRY(pack_attn(e, s.attn)); SRGD_TRY(pack_conv(e, s.resample));
  }
  e->mx2_pack = e->mx2_exact_tail < 1;
  SRGD_TRY(pack_res(e, e->final_rb));
  e->mx2_pack = true;
  for (auto& t : e->wt) { std::vector<float>().swap(t.data); }
  e->finalized = true;
  return 0;
}

// the U-Net evaluation of the forward entries once ct_api and d_rows are set
static int unet_forward_with_rows(srgd_engine* e, const float* xin, const float* cond, float* eps_out, int B, int H, int W,
                                  hipStream_t st) {
  void* x0 = e->pool.get((size_t)B * H * W * e->dim * e->es);
  if (!x0) return -1;
  {
    Prof p(e, KC_INIT, st);
    void* padded = e->pool.get((size_t)B * (H + 6) * (W + 8) * 8 * e->es);
    if (!padded) return -1;
    SRGD_TRY(init_gather_from_nchw(xin, cond, B, H, W, padded, e->bf16, st));
    SRGD_TRY(run_init7(e, padded, B, H, W, x0, st));
    e->pool.put(padded);
  }
  Ctx x{e, B, H, W, e->d_rows, e->ct_api.table, st};
  void* act = nullptr;
  SRGD_TRY(unet_body(x, x0, &act));
  { Prof p(e, KC_FINAL, st); SRGD_TRY(final_conv_to_nchw(act, B, H, W, e->dim, e->final_w, e->final_b, eps_out, e->bf16, st)); }
  e->pool.put(act);
  e->pool.put(x0);
  return 0;
}

int srgd_unet_forward(srgd_engine* e, const float* xin, const float* cond, const float* log_snr_host, int class_id,
                      float* eps_out, int B, int H, int W, void* stream) {
  if (!e || !e->finalized) SRGD_FAIL("srgd_unet_forward: engine has no weights");
  if (class_id >= 0 && e->cfg.num_classes <= 0) SRGD_FAIL("class label given but the U-Net has no class embedding");
  hipStream_t st = (hipStream_t)stream;
  SRGD_HIP(hipSetDevice(e->cfg.device));
  e->pool.reset_busy();
  SRGD_TRY(ensure_scratch(e, B, H, W));
  SRGD_TRY(compute_conditioning(e, e->ct_api, log_snr_host, B, &class_id, 1, st));
  hipLaunchKernelGGL(rows_api_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, e->d_rows, B, class_id >= 0 ? 0 : 1);
  return unet_forward_with_rows(e, xin, cond, eps_out, B, H, W, st);
}

int srgd_unet_forward_labels(srgd_engine* e, const float* xin, const float* cond, const float* log_snr_host,
                             const int32_t* class_ids_host, float* eps_out, int B, int H, int W, void* stream) {
  if (!e || !e->finalized) SRGD_FAIL("srgd_unet_forward_labels: engine has no weights");
  if (!class_ids_host || B < 1) SRGD_FAIL("srgd_unet_forward_labels: null argument");
  if (e->cfg.num_classes <= 0) SRGD_FAIL("class label given but the U-Net has no class embedding");
  std::vector<int> labels;
  SRGD_TRY(label_slots(e, class_ids_host, B, labels, e->slots_api_host));
  const int K = (int)labels.size();
  hipStream_t st = (hipStream_t)stream;
  SRGD_HIP(hipSetDevice(e->cfg.device));
  e->pool.reset_busy();
  SRGD_TRY(ensure_scratch(e, B, H, W));
  SRGD_TRY(ensure(e, &e->d_slots_api, &e->slots_api_cap, (size_t)B));
  SRGD_HIP(hipMemcpyAsync(e->d_slots_api, e->slots_api_host.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
  SRGD_TRY(compute_conditioning(e, e->ct_api, log_snr_host, B, labels.data(), K, st));
  hipLaunchKernelGGL(rows_api_labels_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, e->d_rows, B, K + 1, e->d_slots_api);
  return unet_forward_with_rows(e, xin, cond, eps_out, B, H, W, st);
}

// Probes of the conditioning path (srgd_hip_kernels.h): compute_conditioning on a table of the call's own, and the table's columns
int srgd_k_conditioning_table(void* engine, const float* log_snr_host, int n, const int32_t* class_ids_host, int K,
                              float* table_host, void* stream) {
  srgd_engine* e = (srgd_engine*)engine;
  if (!e || !log_snr_host || !class_ids_host || !table_host) SRGD_FAIL("srgd_k_conditioning_table: null argument");
  if (!e->finalized) SRGD_FAIL("srgd_k_conditioning_table: engine has no weights");
  if (n < 1 || K < 1) SRGD_FAIL("srgd_k_conditioning_table: empty table");
  if (class_ids_host[0] >= 0 && e->cfg.num_classes <= 0) SRGD_FAIL("class label given but the U-Net has no class embedding");
  hipStream_t st = (hipStream_t)stream;
  SRGD_HIP(hipSetDevice(e->cfg.device));
  std::vector<int> ids(class_ids_host, class_ids_host + K);
  CondTable ct;
  const bool prof_on = e->prof_on;           // a probe leaves no record in the engine's profile
  e->prof_on = false;
  int rc = compute_conditioning(e, ct, log_snr_host, n, ids.data(), K, st);
  e->prof_on = prof_on;
  if (rc == 0 && hipMemcpyAsync(table_host, ct.table, (size_t)(K + 1) * n * e->ss_stride * 4, hipMemcpyDeviceToHost, st) != hipSuccess) rc = -2;
  if (hipStreamSynchronize(st) != hipSuccess && rc == 0) rc = -2;
  for (float* q : {ct.table, ct.ls, ct.feat, ct.h1, ct.t1, ct.trows, ct.c1, ct.c2})
    if (q) hipFree(q);
  if (rc == -2) SRGD_FAIL("srgd_k_conditioning_table: copying the table back failed");
  return rc;
}

int srgd_k_conditioning_layout(void* engine, int* ss_stride, int* n_blocks, int index, char* name, size_t name_cap, int* ss_offset,
                               int* Cout) {
  const srgd_engine* e = (const srgd_engine*)engine;
  if (!e) SRGD_FAIL("srgd_k_conditioning_layout: null argument");
  if (ss_stride) *ss_stride = e->ss_stride;
  if (n_blocks) *n_blocks = (int)e->all_rb.size();
  if (index < 0) return 0;
  if (index >= (int)e->all_rb.size()) SRGD_FAIL("srgd_k_conditioning_layout: bad index");
  const ResW* r = e->all_rb[index];
  if (name && name_cap) {
    const std::string& w = e->wt[r->mlp.wi].name;            // "<block>.mlp.1.weight"
    const std::string block = w.substr(0, w.size() - std::strlen(".mlp.1.weight"));
    std::strncpy(name, block.c_str(), name_cap - 1);
    name[name_cap - 1] = 0;
  }
  if (ss_offset) *ss_offset = r->ss_offset;
  if (Cout) *Cout = r->Cout;
  return 0;
}

// one image of a run as the begin entries receive it: its geometry, its two tile grids (host [n][2] = (y, x)) and its noise class
struct ImageIn { srgd_sampler_image g; const int32_t* tiles_even; const int32_t* tiles_odd; };

// shared by the DDPM and the EDM sampler: geometry checks, tile lists, image records, condition canvas, conditioning table for
// the n_times "time" inputs of the run (rows 2i: with the class embedding, 2i+1: without)
static int sampler_begin_common(srgd_engine* e, int tile, const std::vector<ImageIn>& ims, const float* cond01, float* cond_canvas,
                                int n_steps, const float* times_host, int n_times, int class_id, hipStream_t st) {
  if (!e || !e->finalized) SRGD_FAIL("srgd_sampler_begin: engine has no weights");
  if (!cond01 || !cond_canvas || !times_host) SRGD_FAIL("srgd_sampler_begin: null argument");
  if (class_id >= 0 && e->cfg.num_classes <= 0) SRGD_FAIL("class label given but the U-Net has no class embedding");
  if (tile <= 0 || n_steps <= 0 || ims.empty()) SRGD_FAIL("srgd_sampler_begin: bad geometry");
  std::vector<ImageDesc> recs;
  std::vector<srgd_engine::NoiseClass> classes;
  std::vector<int> class_n[2];
  std::vector<int32_t> tl[2];                // device tile lists are image-major [(y, x, image)]: one U-Net batch may span images
  long long canvas_off = 0, cond_off = 0, cnoise_off = 0;
  int max_local[2] = {0, 0};
  long max_canvas = 0, max_image = 0;
  for (size_t im = 0; im < ims.size(); ++im) {
    const srgd_sampler_image& g = ims[im].g;
    if (g.H <= 0 || g.W <= 0 || g.Hp < tile || g.Wp < tile || g.n_even <= 0 || g.n_odd <= 0 || !ims[im].tiles_even || !ims[im].tiles_odd ||
        g.left < 0 || g.top < 0 || g.left + g.W > g.Wp || g.top + g.H > g.Hp || g.inner_l < 0 || g.inner_t < 0 ||
        g.inner_l > g.inner_r || g.inner_t > g.inner_b || g.inner_r > g.Wp || g.inner_b > g.Hp)
      SRGD_FAIL("srgd_sampler_begin: bad geometry");
    // F.pad(mode='reflect') requires pad < input size (model.py:3303 raises otherwise)
    const int pl = g.left, pr = g.Wp - g.left - g.W, pt = g.top, pb = g.Hp - g.top - g.H;
    if (pl >= g.W || pr >= g.W || pt >= g.H || pb >= g.H)
      SRGD_FAIL("Padding size should be less than the corresponding input dimension (reflect pad)");
    // noise classes are numbered in order of first appearance; one class = one canvas size = one draw sequence
    const int k = g.noise_class;
    if (k < 0 || k > (int)classes.size()) SRGD_FAIL("srgd_sampler_begin_images: noise classes must be numbered 0, 1, ... in order of first appearance");
    if (k == (int)classes.size()) {
      classes.push_back({g.Hp, g.Wp, cnoise_off});
      class_n[0].push_back(g.n_even);
      class_n[1].push_back(g.n_odd);
      cnoise_off += 3LL * g.Hp * g.Wp;
    } else if (classes[k].Hp != g.Hp || classes[k].Wp != g.Wp || class_n[0][k] != g.n_even || class_n[1][k] != g.n_odd) {
      SRGD_FAIL("srgd_sampler_begin_images: images of one noise class must share their canvas and tile grids");
    }
    ImageDesc d{};
    d.canvas_off = canvas_off; d.cond_off = cond_off; d.cnoise_off = classes[k].cnoise_off;
    d.Hp = g.Hp; d.Wp = g.Wp; d.left = g.left; d.top = g.top; d.H = g.H; d.W = g.W;
    d.inner_l = g.inner_l; d.inner_t = g.inner_t; d.inner_r = g.inner_r; d.inner_b = g.inner_b;
    d.noise_class = k;
    for (int par = 0; par < 2; ++par) {
      const int nl = par ? g.n_odd : g.n_even;
      const int32_t* src = par ? ims[im].tiles_odd : ims[im].tiles_even;
      d.tile0[par] = (int)(tl[par].size() / 3);
      d.tnoise0[par] = 0;
      for (int j = 0; j < k; ++j) d.tnoise0[par] += class_n[par][j];
      for (int t = 0; t < nl; ++t) {
        const int y = src[2 * t], x = src[2 * t + 1];
        if (y < 0 || x < 0 || y + tile > g.Hp || x + tile > g.Wp)
          SRGD_FAIL(par ? "srgd_sampler_begin: odd-grid tile outside the canvas" : "srgd_sampler_begin: even-grid tile outside the canvas");
        tl[par].insert(tl[par].end(), {y, x, (int32_t)im});
      }
      max_local[par] = std::max(max_local[par], nl);
    }
    recs.push_back(d);
    canvas_off += 3LL * g.Hp * g.Wp;
    cond_off += 3LL * g.H * g.W;
    max_canvas = std::max(max_canvas, 3L * g.Hp * g.Wp);
    max_image = std::max(max_image, 3L * g.H * g.W);
  }
  SRGD_HIP(hipSetDevice(e->cfg.device));
  drop_step_graphs(e);                       // graphs bake in canvas / table / tile-list pointers of one run
  e->n_steps = n_steps;
  e->run_class = class_id;
  e->n_labels = 1;
  e->run_labels = e->run_stepped = e->run_seeded = false;
  e->run_times.assign(times_host, times_host + n_times);
  e->images = recs;
  e->classes = classes;
  e->class_canvas_elems = (size_t)cnoise_off;
  for (int par = 0; par < 2; ++par) {
    e->class_n[par] = class_n[par];
    e->n_grid[par] = (int)(tl[par].size() / 3);
    e->max_local[par] = max_local[par];
  }
  e->max_canvas = max_canvas;
  e->max_image = max_image;
  SRGD_TRY(ensure(e, &e->d_tiles_even, &e->tiles_cap_even, tl[0].size()));
  SRGD_TRY(ensure(e, &e->d_tiles_odd, &e->tiles_cap_odd, tl[1].size()));
  SRGD_TRY(ensure(e, &e->d_images, &e->images_cap, recs.size()));
  SRGD_HIP(hipMemcpyAsync(e->d_tiles_even, tl[0].data(), tl[0].size() * 4, hipMemcpyHostToDevice, st));
  SRGD_HIP(hipMemcpyAsync(e->d_tiles_odd, tl[1].data(), tl[1].size() * 4, hipMemcpyHostToDevice, st));
  SRGD_HIP(hipMemcpyAsync(e->d_images, recs.data(), recs.size() * sizeof(ImageDesc), hipMemcpyHostToDevice, st));
  { Prof p(e, KC_CANVAS, st);
    SRGD_TRY(canvas_prepare_cond(cond01, e->d_images, (int)recs.size(), max_canvas, cond_canvas, st)); }
  SRGD_TRY(compute_conditioning(e, e->ct_sampler, times_host, n_times, &class_id, 1, st));
  // the host arrays (ours and the caller's) may be reused right after this returns
  SRGD_HIP(hipStreamSynchronize(st));
  return 0;
}

// a same-sized run: n_images records of one geometry, one noise class
static int sampler_begin_uniform(srgd_engine* e, const srgd_sampler_geometry* g, const float* cond01, float* cond_canvas,
                                 const int32_t* tiles_even_host, const int32_t* tiles_odd_host, int n_steps,
                                 const float* times_host, int n_times, int class_id, hipStream_t st) {
  if (!g || !tiles_even_host || !tiles_odd_host) SRGD_FAIL("srgd_sampler_begin: null argument");
  if (g->n_images < 1) SRGD_FAIL("srgd_sampler_begin: bad geometry");
  const srgd_sampler_image one{g->H, g->W, g->Hp, g->Wp, g->left, g->top, g->inner_l, g->inner_t, g->inner_r, g->inner_b,
                               g->n_even, g->n_odd, 0};
  const std::vector<ImageIn> ims(g->n_images, ImageIn{one, tiles_even_host, tiles_odd_host});
  SRGD_TRY(sampler_begin_common(e, g->tile, ims, cond01, cond_canvas, n_steps, times_host, n_times, class_id, st));
  e->geo = *g;
  e->run_mixed = false;
  return 0;
}

int srgd_sampler_begin(srgd_engine* e, const srgd_sampler_geometry* g, const float* cond01, float* cond_canvas,
                       const int32_t* tiles_even_host, const int32_t* tiles_odd_host, int n_steps,
                       const srgd_step_scalars* scalars_host, const float* log_snr_host, int class_id, void* stream) {
  if (!scalars_host) SRGD_FAIL("srgd_sampler_begin: null argument");
  hipStream_t st = (hipStream_t)stream;
  static_assert(sizeof(StepScalars) == sizeof(srgd_step_scalars), "step scalar layout");
  if (e && n_steps > 0) SRGD_TRY(upload_step_scalars(e, &e->d_sc, &e->sc_cap, n_steps, scalars_host, st));
  SRGD_TRY(sampler_begin_uniform(e, g, cond01, cond_canvas, tiles_even_host, tiles_odd_host, n_steps, log_snr_host, n_steps,
                                 class_id, st));
  e->run_active = true;
  e->run_is_edm = false;
  return 0;
}

int srgd_sampler_begin_images(srgd_engine* e, int tile, int n_images, const srgd_sampler_image* images, const float* cond01,
                              float* cond_canvas, const int32_t* tiles_even_host, const int32_t* tiles_odd_host, int n_steps,
                              const srgd_step_scalars* scalars_host, const float* log_snr_host, int class_id, void* stream) {
  if (!images || !scalars_host || !tiles_even_host || !tiles_odd_host) SRGD_FAIL("srgd_sampler_begin_images: null argument");
  if (n_images < 1) SRGD_FAIL("srgd_sampler_begin_images: n_images must be >= 1");
  hipStream_t st = (hipStream_t)stream;
  std::vector<ImageIn> ims;
  size_t oe = 0, oo = 0;
  for (int i = 0; i < n_images; ++i) {
    if (images[i].n_even <= 0 || images[i].n_odd <= 0) SRGD_FAIL("srgd_sampler_begin: bad geometry");
    ims.push_back(ImageIn{images[i], tiles_even_host + 2 * oe, tiles_odd_host + 2 * oo});
    oe += images[i].n_even;
    oo += images[i].n_odd;
  }
  if (e && n_steps > 0) SRGD_TRY(upload_step_scalars(e, &e->d_sc, &e->sc_cap, n_steps, scalars_host, st));
  SRGD_TRY(sampler_begin_common(e, tile, ims, cond01, cond_canvas, n_steps, log_snr_host, n_steps, class_id, st));
  e->geo = srgd_sampler_geometry{};
  e->geo.tile = tile;
  e->geo.n_images = n_images;
  e->run_mixed = true;
  e->run_active = true;
  e->run_is_edm = false;
  return 0;
}

int srgd_edm_begin(srgd_engine* e, const srgd_sampler_geometry* g, const float* cond01, float* cond_canvas,
                   const int32_t* tiles_even_host, const int32_t* tiles_odd_host, int n_steps,
                   const srgd_edm_scalars* scalars_host, const float* c_noise_host, int class_id, void* stream) {
  if (!scalars_host) SRGD_FAIL("srgd_edm_begin: null argument");
  hipStream_t st = (hipStream_t)stream;
  static_assert(sizeof(EdmScalars) == sizeof(srgd_edm_scalars), "EDM scalar layout");
  if (e && n_steps > 0) SRGD_TRY(upload_step_scalars(e, &e->d_edm, &e->edm_cap, n_steps, scalars_host, st));
  // two network evaluations per step: rows 4i..4i+1 for c_noise(sigma_hat_i), 4i+2..4i+3 for c_noise(sigma_next_i)
  SRGD_TRY(sampler_begin_uniform(e, g, cond01, cond_canvas, tiles_even_host, tiles_odd_host, n_steps, c_noise_host,
                                 2 * n_steps, class_id, st));
  e->run_active = true;
  e->run_is_edm = true;
  return 0;
}

int srgd_sampler_image_labels(srgd_engine* e, const int32_t* class_ids_host, int n_images, void* stream) {
  if (!e || !e->run_active) SRGD_FAIL("srgd_sampler_image_labels: call srgd_sampler_begin, srgd_sampler_begin_images or srgd_edm_begin first");
  if (!class_ids_host) SRGD_FAIL("srgd_sampler_image_labels: null argument");
  if (e->cfg.num_classes <= 0) SRGD_FAIL("class label given but the U-Net has no class embedding");
  if (n_images != (int)e->images.size()) SRGD_FAIL("srgd_sampler_image_labels: one label per image of the run");
  if (e->run_stepped) SRGD_FAIL("srgd_sampler_image_labels: the run has taken a step (labels are set before the first)");
  std::vector<int> labels, slots;
  SRGD_TRY(label_slots(e, class_ids_host, n_images, labels, slots));
  hipStream_t st = (hipStream_t)stream;
  SRGD_HIP(hipSetDevice(e->cfg.device));
  drop_step_graphs(e);                       // graphs bake in the table pointer and the rows per step
  SRGD_TRY(ensure(e, &e->d_slots, &e->slots_cap, (size_t)n_images));
  e->slots_host = slots;
  SRGD_HIP(hipMemcpyAsync(e->d_slots, e->slots_host.data(), (size_t)n_images * sizeof(int), hipMemcpyHostToDevice, st));
  SRGD_TRY(compute_conditioning(e, e->ct_sampler, e->run_times.data(), (int)e->run_times.size(), labels.data(), (int)labels.size(), st));
  e->n_labels = (int)labels.size();
  e->run_labels = true;
  e->run_class = labels[0];
  SRGD_HIP(hipStreamSynchronize(st));
  return 0;
}

// Probe of launch_step_rows (srgd_hip_kernels.h): the launch a sampler step makes for one U-Net batch, into a buffer of the call's own
int srgd_k_step_rows(void* engine, int parity, int nb, int nt, int first, int ev, int pass1_null, int32_t* rows_host, void* stream) {
  srgd_engine* e = (srgd_engine*)engine;
  if (!e || !rows_host) SRGD_FAIL("srgd_k_step_rows: null argument");
  if (!e->run_active) SRGD_FAIL("srgd_k_step_rows: call srgd_sampler_begin, srgd_sampler_begin_images or srgd_edm_begin first");
  const int par = parity & 1;
  if (nt < 1 || (nb != nt && nb != 2 * nt) || first < 0 || first + nt > e->n_grid[par] || ev < 0 || ev > 1)
    SRGD_FAIL("srgd_k_step_rows: the batch is one or two passes of tiles [first, first + nt) of the parity's grid, ev is 0 or 1");
  hipStream_t st = (hipStream_t)stream;
  SRGD_HIP(hipSetDevice(e->cfg.device));
  int* tmp = nullptr;
  SRGD_HIP(hipMalloc((void**)&tmp, (size_t)nb * sizeof(int)));
  int* const run_rows = e->d_rows;           // the run keeps its own buffer and its contents
  e->d_rows = tmp;
  launch_step_rows(e, nb, nt, par ? e->d_tiles_odd : e->d_tiles_even, first, ev, pass1_null != 0 ? 0x2 : 0x0, st);
  e->d_rows = run_rows;
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipMemcpyAsync(rows_host, tmp, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  (void)hipFree(tmp);
  SRGD_HIP(err);
  return 0;
}

int srgd_sampler_noise_seeds(srgd_engine* e, const uint64_t* seeds_host, int n_classes, void* stream) {
  if (!e || !e->run_active) SRGD_FAIL("srgd_sampler_noise_seeds: call srgd_sampler_begin or srgd_sampler_begin_images first");
  if (!seeds_host) SRGD_FAIL("srgd_sampler_noise_seeds: null argument");
  if (e->run_is_edm) SRGD_FAIL("srgd_sampler_noise_seeds: not available on an EDM run (its step kernels address one shared noise canvas)");
  if (n_classes != (int)e->classes.size()) SRGD_FAIL("srgd_sampler_noise_seeds: one seed per noise class of the run");
  if (e->run_stepped) SRGD_FAIL("srgd_sampler_noise_seeds: the run has taken a step (seeds are set before the first)");
  hipStream_t st = (hipStream_t)stream;
  SRGD_HIP(hipSetDevice(e->cfg.device));
  drop_step_graphs(e);                       // graphs bake in which draws a step launches
  const size_t K = (size_t)n_classes, tile_elems = (size_t)3 * e->geo.tile * e->geo.tile;
  e->streams_host.assign(3 * K, PhiloxStream{});
  for (int use = 0; use < 3; ++use) {
    long long off = 0;
    e->stream_max_n[use] = 0;
    for (size_t k = 0; k < K; ++k) {
      const long long n = use < 2 ? (long long)e->class_n[use][k] * (long long)tile_elems : 3LL * e->classes[k].Hp * e->classes[k].Wp;
      e->streams_host[use * K + k] = PhiloxStream{use < 2 ? off : e->classes[k].cnoise_off, n, (unsigned long long)seeds_host[k]};
      off += n;
      e->stream_max_n[use] = std::max(e->stream_max_n[use], (size_t)n);
    }
    if (use < 2) e->class_tiles[use] = (int)(off / (long long)tile_elems);
  }
  // every buffer a seeded step or q_start draws into, before any capture
  SRGD_TRY(ensure(e, &e->d_streams, &e->streams_cap, 3 * K));
  SRGD_TRY(ensure(e, &e->rng_tiles, &e->rng_tiles_cap, (size_t)std::max(e->class_tiles[0], e->class_tiles[1]) * tile_elems));
  SRGD_TRY(ensure(e, &e->rng_canvas, &e->rng_canvas_cap, e->class_canvas_elems));
  SRGD_HIP(hipMemcpyAsync(e->d_streams, e->streams_host.data(), 3 * K * sizeof(PhiloxStream), hipMemcpyHostToDevice, st));
  SRGD_HIP(hipStreamSynchronize(st));
  e->run_seeded = true;
  return 0;
}

// all launches of one EDM step (model.py:2377-2455); step-dependent values come through e->d_step
static int edm_step_launch(srgd_engine* e, bool last, int parity, int tile_first, int tile_count, bool ring, float* img,
                           const float* cond_canvas, float* x_start, float* work, const float* noise_canvas,
                           const float* ring_noise_canvas, int passes, int guidance_kind, float guidance_scale, int sub_batch,
                           uint64_t seed, hipStream_t st) {
  const srgd_sampler_geometry& g = e->geo;
  const int n_local = parity ? g.n_odd : g.n_even;
  const int n = tile_first + tile_count;               // this call covers tiles [tile_first, n) of the image-major list
  const int* tiles = parity ? e->d_tiles_odd : e->d_tiles_even;
  const size_t canvas1 = (size_t)3 * g.Hp * g.Wp, canvas_elems = canvas1 * g.n_images;
  const float* z = noise_canvas;
  if (!z) {
    Prof p(e, KC_CANVAS, st);
    SRGD_TRY(philox_normal(e->rng_tiles, canvas1, seed, 2ull << 32, e->d_step, st));
    z = e->rng_tiles;
  }
  for (int first = tile_first; first < n; first += sub_batch) {
    const TileBatch tb{tiles, first, std::min(sub_batch, n - first), g.Hp, g.Wp, g.tile, n_local, e->d_images, parity};
    for (int ep = 0; ep < (last ? 1 : 2); ++ep)      // Euler evaluation from the canvas, Heun evaluation from the Euler result in `work`
      SRGD_TRY(eval_tile_batch(
          e, tb, StepEval{passes, guidance_kind, guidance_scale, img, x_start, ep, 2}, st,
          [&](int mask, void* padded) {
            return init_gather_from_canvas_edm(ep == 0 ? img : work, ep == 0 ? z : nullptr, cond_canvas, tb, passes, mask, e->d_edm,
                                               e->d_step, ep, padded, e->bf16, st);
          },
          [&](FinalStepArgs& fa) {
            fa.noise = z;
            return final_step_edm(fa, e->d_edm, work, canvas_elems, ep, tb, e->bf16, st);
          }));
  }
  if (parity == 1 && ring) {
    Prof p(e, KC_CANVAS, st);
    const float* nc = ring_noise_canvas;
    if (!nc) {
      SRGD_TRY(philox_normal(e->rng_canvas, canvas1, seed, (1ull << 32) | 0x80000000ull, e->d_step, st));
      nc = e->rng_canvas;
    }
    SRGD_TRY(canvas_ring_renoise(img, e->d_images, g.n_images, e->max_canvas, nc, &e->d_edm[0].ring_sigma,
                                 (int)(sizeof(EdmScalars) / sizeof(float)), e->d_step, st));
  }
  return 0;
}

// One EDM step over every tile of grid (step % 2): Euler evaluation at sigma_hat, Heun correction at sigma_next (skipped on the
// last step), odd-step ring re-noise.  In device-noise mode the step is captured and replayed like the DDPM step.
int srgd_edm_step(srgd_engine* e, int step, float* img, const float* cond_canvas, float* x_start, float* work,
                  const float* noise_canvas, const float* ring_noise_canvas, int passes, int guidance_kind,
                  float guidance_scale, int sub_batch, uint64_t seed, void* stream) {
  return srgd_edm_step_tiles(e, step, 0, -1, 1, img, cond_canvas, x_start, work, noise_canvas, ring_noise_canvas, passes,
                             guidance_kind, guidance_scale, sub_batch, seed, stream);
}

// The per-rank unit of a canvas shared by several GPUs (as srgd_sampler_step_tiles for the DDPM loop): tiles
// [tile_first, tile_first + tile_count) of the step's grid; the two scratch canvases in `work` are touched at those tiles only.
int srgd_edm_step_tiles(srgd_engine* e, int step, int tile_first, int tile_count, int do_ring, float* img,
                        const float* cond_canvas, float* x_start, float* work, const float* noise_canvas,
                        const float* ring_noise_canvas, int passes, int guidance_kind, float guidance_scale, int sub_batch,
                        uint64_t seed, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  StepPlan p;
  SRGD_TRY(step_prologue(e, "srgd_edm_step", /*edm=*/true, /*null_arg=*/!img || !cond_canvas || !work, step, tile_first, tile_count, passes,
                         guidance_kind, sub_batch, &p));
  const bool ring = do_ring != 0;
  const size_t canvas1 = (size_t)3 * e->geo.Hp * e->geo.Wp;
  if (!noise_canvas) SRGD_TRY(ensure(e, &e->rng_tiles, &e->rng_tiles_cap, canvas1));
  if (!ring_noise_canvas && p.parity == 1 && ring) SRGD_TRY(ensure(e, &e->rng_canvas, &e->rng_canvas_cap, canvas1));
  SRGD_TRY(set_device_step(e, step, st));
  const bool graphable = e->use_graphs && !e->prof_on && !noise_canvas && !ring_noise_canvas;
  if (!graphable)
    return edm_step_launch(e, p.last, p.parity, p.tile_first, p.tile_count, ring, img, cond_canvas, x_start, work, noise_canvas,
                           ring_noise_canvas, passes, guidance_kind, guidance_scale, p.sub_batch, seed, st);
  srgd_engine::StepKey key{};
  key.mode = 1; key.work = work;
  key.parity = p.parity; key.last = p.last; key.tile_first = p.tile_first; key.tile_count = p.tile_count; key.sub_batch = p.sub_batch;
  key.passes = passes; key.kind = guidance_kind; key.scale = guidance_scale; key.seed = seed; key.ring = ring;
  key.img = img; key.cond = cond_canvas; key.xs = x_start;
  return run_step_through_graph(e, key, st, [&](hipStream_t s2) {
    return edm_step_launch(e, p.last, p.parity, p.tile_first, p.tile_count, ring, img, cond_canvas, x_start, work, nullptr, nullptr,
                           passes, guidance_kind, guidance_scale, p.sub_batch, seed, s2);
  });
}

// One DPM-Solver++(2M) step (reference sample_using_dpmpp, model.py:2517-2547): one network evaluation per tile at sigma_i,
// multistep update against the previous step's denoised canvas.  Deterministic (no noise), launched eagerly.
int srgd_edm_dpmpp_step(srgd_engine* e, int step, float* img, const float* cond_canvas, float* x_start, float* old_denoised,
                        int passes, int guidance_kind, float guidance_scale, int sub_batch, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  StepPlan p;
  SRGD_TRY(step_prologue(e, "srgd_edm_dpmpp_step", /*edm=*/true, /*null_arg=*/!img || !cond_canvas || !old_denoised, step, 0, -1, passes,
                         guidance_kind, sub_batch, &p));
  SRGD_TRY(set_device_step(e, step, st));
  const srgd_sampler_geometry& g = e->geo;
  const int* tiles = p.parity ? e->d_tiles_odd : e->d_tiles_even;
  const size_t canvas_elems = (size_t)3 * g.Hp * g.Wp * g.n_images;
  // conditioning rows of evaluation 0 (c_noise at sigma_i) of the two the table holds per step; gather and final step in their
  // DPM-Solver++ form (edm_pass 2)
  const StepEval ev{passes, guidance_kind, guidance_scale, img, x_start, 0, 2};
  for (int first = 0; first < p.tile_count; first += p.sub_batch) {
    const TileBatch tb{tiles, first, std::min(p.sub_batch, p.tile_count - first), g.Hp, g.Wp, g.tile, p.parity ? g.n_odd : g.n_even,
                       e->d_images, p.parity};
    SRGD_TRY(eval_tile_batch(
        e, tb, ev, st,
        [&](int mask, void* padded) {
          return init_gather_from_canvas_edm(img, nullptr, cond_canvas, tb, passes, mask, e->d_edm, e->d_step, 2, padded, e->bf16, st);
        },
        [&](FinalStepArgs& fa) { return final_step_edm(fa, e->d_edm, old_denoised, canvas_elems, 2, tb, e->bf16, st); }));
  }
  return 0;
}

// all launches of one DDPM step; step-dependent values come through e->d_step (set by the caller on the stream)
static int sampler_step_launch(srgd_engine* e, bool last, int parity, int tile_first, int tile_count, bool ring, float* img,
                               const float* cond_canvas, float* x_start, const float* noise_tiles,
                               const float* noise_canvas, int passes, int guidance_kind, float guidance_scale,
                               float class_scale, int sub_batch, uint64_t seed, hipStream_t st) {
  const srgd_sampler_geometry& g = e->geo;
  const int* tiles = parity ? e->d_tiles_odd : e->d_tiles_even;
  const int n = tile_first + tile_count;               // this call covers tiles [tile_first, n) of the image-major list
  const size_t tile_elems = (size_t)3 * g.tile * g.tile;
  const float* nz = nullptr;
  if (!last) {
    nz = noise_tiles;
    if (!nz) {   // the largest image's worth of tile noise, shared by every image (counter-based: a prefix of it is what a
                 // smaller image draws alone) and independent of sub_batch
      Prof p(e, KC_CANVAS, st);
      if (e->run_seeded)   // per-class seeds: each class's own tiles from its own seed, concatenated in class order, one launch
        SRGD_TRY(philox_normal_streams(e->rng_tiles, e->d_streams + (size_t)parity * e->classes.size(), (int)e->classes.size(),
                                       e->stream_max_n[parity], 1ull << 32, e->d_step, st));
      else
        SRGD_TRY(philox_normal(e->rng_tiles, (size_t)e->max_local[parity] * tile_elems, seed, 1ull << 32, e->d_step, st));
      nz = e->rng_tiles;
    }
  }
  const StepEval ev{passes, guidance_kind, guidance_scale, img, x_start, 0, 1, class_scale};
  for (int first = tile_first; first < n; first += sub_batch) {
    const TileBatch tb{tiles, first, std::min(sub_batch, n - first), g.Hp, g.Wp, g.tile, 0, e->d_images, parity};
    SRGD_TRY(eval_tile_batch(
        e, tb, ev, st,
        [&](int mask, void* padded) { return init_gather_from_canvas(img, cond_canvas, tb, passes, mask, padded, e->bf16, st); },
        [&](FinalStepArgs& fa) {
          fa.noise = nz;
          fa.noise_per_class = (noise_tiles || e->run_seeded) ? 1 : 0;
          fa.sc = e->d_sc;
          if (e->prof_on) {
            const double px = (double)tb.ntiles * g.tile * g.tile;
            e->fam_bytes[KC_FINAL] += px * passes * (fa.eps4 ? 16.0 : (double)e->dim * e->es) + px * 12.0 * (3.0 + (x_start ? 1.0 : 0.0));
          }
          return final_step(fa, tb, e->bf16, st);
        }));
  }
  if (parity == 1 && ring) {
    Prof p(e, KC_CANVAS, st);
    const float* nc = noise_canvas;
    if (!nc) {   // one draw per noise class (canvas size): what each of its images draws alone
      if (e->run_seeded)
        SRGD_TRY(philox_normal_streams(e->rng_canvas, e->d_streams + 2 * e->classes.size(), (int)e->classes.size(),
                                       e->stream_max_n[2], (1ull << 32) | 0x80000000ull, e->d_step, st));
      else
        for (const auto& k : e->classes)
          SRGD_TRY(philox_normal(e->rng_canvas + k.cnoise_off, (size_t)3 * k.Hp * k.Wp, seed, (1ull << 32) | 0x80000000ull,
                                 e->d_step, st));
      nc = e->rng_canvas;
    }
    SRGD_TRY(canvas_ring_renoise(img, e->d_images, (int)e->images.size(), e->max_canvas, nc, &e->d_sc[0].sigma_next,
                                 (int)(sizeof(StepScalars) / sizeof(float)), e->d_step, st));
  }
  return 0;
}

static void drop_step_graphs(srgd_engine* e) {
  for (auto& sg : e->graphs) {
    if (sg.exec) (void)hipGraphExecDestroy(sg.exec);
    if (sg.graph) (void)hipGraphDestroy(sg.graph);
  }
  e->graphs.clear();
}

int srgd_sampler_step(srgd_engine* e, int step, float* img, const float* cond_canvas, float* x_start,
                      const float* noise_tiles, const float* noise_canvas, int passes, int guidance_kind,
                      float guidance_scale, int sub_batch, uint64_t seed, void* stream) {
  return srgd_sampler_step_tiles(e, step, 0, -1, 1, img, cond_canvas, x_start, noise_tiles, noise_canvas, passes,
                                 guidance_kind, guidance_scale, sub_batch, seed, stream);
}

// The joint form of srgd_sampler_step / _step_tiles (srgd_hip.h): passes == 3, and guidance_kind holds the bits of the class scale
static float joint_class_scale(int guidance_kind) {
  float v;
  static_assert(sizeof(v) == sizeof(guidance_kind), "the class scale travels in the int");
  std::memcpy(&v, &guidance_kind, sizeof(v));
  return v;
}

int srgd_sampler_step_tiles(srgd_engine* e, int step, int tile_first, int tile_count, int do_ring, float* img,
                            const float* cond_canvas, float* x_start, const float* noise_tiles,
                            const float* noise_canvas, int passes, int guidance_kind, float guidance_scale,
                            int sub_batch, uint64_t seed, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const bool joint = passes == 3 && e && e->run_active && !e->run_is_edm;
  float class_scale = 0.f;
  if (joint) {               // refused before anything of the run is touched
    class_scale = joint_class_scale(guidance_kind);
    guidance_kind = 3;
    // with a scale of exactly 1 its term vanishes and the step is a one- or two-pass step: the caller asks for that
    if (guidance_scale == 1.0f || class_scale == 1.0f)
      SRGD_FAIL("srgd_sampler_step: passes must be 1 or 2 (3 is joint guidance, which needs both scales different from 1)");
    if (e->run_class < 0 && !e->run_labels)
      SRGD_FAIL("srgd_sampler_step: joint guidance on a run begun without a class (the label-dropped pass would repeat the full one)");
    if (!std::isfinite(guidance_scale) || !std::isfinite(class_scale)) SRGD_FAIL("srgd_sampler_step: joint guidance needs finite scales");
  }
  StepPlan p;
  SRGD_TRY(step_prologue(e, "srgd_sampler_step", /*edm=*/false, /*null_arg=*/false, step, tile_first, tile_count, passes, guidance_kind,
                         sub_batch, &p, joint));
  const bool ring = do_ring != 0;
  if (!noise_tiles)    // a seeded run draws every class's tiles (sized by srgd_sampler_noise_seeds already; a no-op then)
    SRGD_TRY(ensure(e, &e->rng_tiles, &e->rng_tiles_cap,
                    (size_t)(e->run_seeded ? e->class_tiles[p.parity] : e->max_local[p.parity]) * 3 * e->geo.tile * e->geo.tile));
  if (!noise_canvas && ring) SRGD_TRY(ensure(e, &e->rng_canvas, &e->rng_canvas_cap, e->class_canvas_elems));
  SRGD_TRY(set_device_step(e, step, st));
  const bool graphable = e->use_graphs && !e->prof_on && !noise_tiles && !noise_canvas;
  if (!graphable)
    return sampler_step_launch(e, p.last, p.parity, p.tile_first, p.tile_count, ring, img, cond_canvas, x_start, noise_tiles,
                               noise_canvas, passes, guidance_kind, guidance_scale, class_scale, p.sub_batch, seed, st);
  srgd_engine::StepKey key{};
  key.mode = 0; key.work = nullptr;
  key.parity = p.parity; key.last = p.last; key.tile_first = p.tile_first; key.tile_count = p.tile_count; key.sub_batch = p.sub_batch;
  key.passes = passes; key.kind = guidance_kind; key.scale = guidance_scale; key.scale2 = class_scale; key.seed = seed; key.ring = ring;
  key.img = img; key.cond = cond_canvas; key.xs = x_start;
  return run_step_through_graph(e, key, st, [&](hipStream_t s2) {
    return sampler_step_launch(e, p.last, p.parity, p.tile_first, p.tile_count, ring, img, cond_canvas, x_start, nullptr, nullptr,
                               passes, guidance_kind, guidance_scale, class_scale, p.sub_batch, seed, s2);
  });
}

int srgd_sampler_exchange_tiles(srgd_engine* e, int parity, int tile_first, int tile_count, float* canvas, float* tiles,
                                int to_canvas, void* stream) {
  if (!e || !e->run_active) SRGD_FAIL("srgd_sampler_exchange_tiles: call srgd_sampler_begin first");
  if (!canvas || !tiles) SRGD_FAIL("srgd_sampler_exchange_tiles: null argument");
  if (e->run_mixed) SRGD_FAIL("srgd_sampler_exchange_tiles: not available after srgd_sampler_begin_images (one canvas per image size)");
  const srgd_sampler_geometry& g = e->geo;
  const int n = (parity & 1 ? g.n_odd : g.n_even) * g.n_images;
  if (tile_first < 0 || tile_count < 0 || tile_first + tile_count > n)
    SRGD_FAIL("srgd_sampler_exchange_tiles: tile range outside the grid");
  if (tile_count == 0) return 0;
  Prof p(e, KC_CANVAS, (hipStream_t)stream);
  TileBatch tb{parity & 1 ? e->d_tiles_odd : e->d_tiles_even, tile_first, tile_count, g.Hp, g.Wp, g.tile,
               parity & 1 ? g.n_odd : g.n_even};
  return canvas_exchange_tiles(canvas, tiles, tb, to_canvas != 0, (hipStream_t)stream);
}

int srgd_sampler_unpack_gathered(srgd_engine* e, int parity, int world, int slice_w, int part_off, int part_w, float* canvas,
                                 const float* gathered, void* stream) {
  if (!e || !e->run_active) SRGD_FAIL("srgd_sampler_unpack_gathered: call srgd_sampler_begin first");
  if (!canvas || !gathered) SRGD_FAIL("srgd_sampler_unpack_gathered: null argument");
  if (e->run_mixed) SRGD_FAIL("srgd_sampler_unpack_gathered: not available after srgd_sampler_begin_images (one canvas per image size)");
  if (world < 1 || slice_w < 1 || part_w < 1 || part_off < 0 || part_off + part_w > slice_w)
    SRGD_FAIL("srgd_sampler_unpack_gathered: the part [part_off, part_off + part_w) must lie inside a slice of slice_w tiles");
  const srgd_sampler_geometry& g = e->geo;
  const int n = (parity & 1 ? g.n_odd : g.n_even) * g.n_images;
  Prof p(e, KC_CANVAS, (hipStream_t)stream);
  TileBatch tb{parity & 1 ? e->d_tiles_odd : e->d_tiles_even, 0, world * part_w, g.Hp, g.Wp, g.tile, parity & 1 ? g.n_odd : g.n_even};
  return canvas_unpack_gathered(canvas, gathered, tb, slice_w, part_off, part_w, n, (hipStream_t)stream);
}

int srgd_sampler_q_start(srgd_engine* e, const float* cond01, const float* noise_canvas, float alpha, float sigma,
                         float* img, uint64_t seed, void* stream) {
  if (!e || !e->run_active) SRGD_FAIL("srgd_sampler_q_start: call srgd_sampler_begin first");
  if (!cond01 || !img) SRGD_FAIL("srgd_sampler_q_start: null argument");
  hipStream_t st = (hipStream_t)stream;
  Prof p(e, KC_CANVAS, st);
  const float* nz = noise_canvas;
  if (!nz) {   // one draw per noise class, as in the ring re-noise
    SRGD_TRY(ensure(e, &e->rng_canvas, &e->rng_canvas_cap, e->class_canvas_elems));
    if (e->run_seeded)
      SRGD_TRY(philox_normal_streams(e->rng_canvas, e->d_streams + 2 * e->classes.size(), (int)e->classes.size(), e->stream_max_n[2],
                                     0, nullptr, st));
    else
      for (const auto& k : e->classes)
        SRGD_TRY(philox_normal(e->rng_canvas + k.cnoise_off, (size_t)3 * k.Hp * k.Wp, seed, 0, nullptr, st));
    nz = e->rng_canvas;
  }
  return canvas_q_start(cond01, e->d_images, (int)e->images.size(), e->max_canvas, nz, alpha, sigma, img, st);
}

int srgd_sampler_end(srgd_engine* e, const float* img, float* out01, void* stream) {
  if (!e || !e->run_active) SRGD_FAIL("srgd_sampler_end: no active run");
  hipStream_t st = (hipStream_t)stream;
  Prof p(e, KC_CANVAS, st);
  SRGD_TRY(canvas_finish(img, e->d_images, (int)e->images.size(), e->max_image, out01, st));
  e->run_active = false;
  return 0;
}

int srgd_randn(srgd_engine* e, float* dst, size_t n, uint64_t seed, uint64_t stream_id, void* stream) {
  if (!e || !dst) SRGD_FAIL("srgd_randn: null argument");
  Prof p(e, KC_CANVAS, (hipStream_t)stream);
  return philox_normal(dst, n, seed, stream_id, nullptr, (hipStream_t)stream);
}

int srgd_profile_begin(srgd_engine* e) {
  if (!e) SRGD_FAIL("null engine");
  for (auto& r : e->prof) { e->ev_free.push_back(r.a); e->ev_free.push_back(r.b); }
  e->prof.clear();
  for (double& f : e->fam_flops) f = 0.0;
  for (double& f : e->fam_bytes) f = 0.0;
  e->prof_on = true;
  return 0;
}

int srgd_profile_end(srgd_engine* e, double* ms, int64_t* launches, double* flops, int n_families) {
  if (!e) SRGD_FAIL("null engine");
  e->prof_on = false;
  SRGD_HIP(hipDeviceSynchronize());
  for (int i = 0; i < n_families && i < KC_COUNT; ++i) {
    if (ms) ms[i] = 0.0;
    if (launches) launches[i] = 0;
    if (flops) flops[i] = e->fam_flops[i];
  }
  for (auto& r : e->prof) {
    float t = 0.f;
    SRGD_HIP(hipEventElapsedTime(&t, r.a, r.b));
    if (r.kc < n_families) { if (ms) ms[r.kc] += t; if (launches) launches[r.kc] += 1; }
    e->ev_free.push_back(r.a); e->ev_free.push_back(r.b);
  }
  e->prof.clear();
  return 0;
}

int srgd_quantize_e4m3(const float* in, float* out, size_t n, float scale) {
  if (!in || !out) SRGD_FAIL("srgd_quantize_e4m3: null argument");
  if (!(scale > 0.f)) SRGD_FAIL("srgd_quantize_e4m3: scale must be positive");
  for (size_t i = 0; i < n; ++i) out[i] = round_through_e4m3(in[i] / scale) * scale;
  return 0;
}

int srgd_profile_bytes(const srgd_engine* e, double* bytes, int n_families) {
  if (!e || !bytes) SRGD_FAIL("srgd_profile_bytes: null argument");
  for (int i = 0; i < n_families && i < KC_COUNT; ++i) bytes[i] = e->fam_bytes[i];
  return 0;
}

int srgd_profile_num_families(void) { return KC_COUNT; }
const char* srgd_profile_family_name(int i) { return (i >= 0 && i < KC_COUNT) ? kFamilyNames[i] : ""; }
int64_t srgd_device_bytes_in_use(const srgd_engine* e) { return e ? e->pool.total + e->weight_bytes : 0; }

}  // extern "C"
