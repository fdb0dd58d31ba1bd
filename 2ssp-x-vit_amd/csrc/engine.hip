// libssp2vit: C ABI (include/ssp2vit.h) + host-side orchestration of the gfx950 kernels.
// Host code is plain C++: shape checks, weight conversion/padding, workspace carving, kernel launches on the
// handle's HIP stream.  No allocation, synchronisation or host<->device copy happens inside the forward
// calls (ssp2_embed / ssp2_layers / ssp2_head), so a caller may capture them into a hipGraph.
#include "../../include/ssp2vit.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "attn.hip.h"
#include "attn_stream.hip.h"
#include "gemm256.hip.h"
#include "misc.hip.h"
#include "patch.hip.h"
#include "preproc.hip.h"

// ------------------------------------------------------------------------------------------------ errors
static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) return fail(SSP2_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));  \
  } while (0)

static inline int ceil_to(int v, int m) { return (v + m - 1) / m * m; }

// slab layout (common.hip.h RowMap): `group` images per slab, slabs padded to a multiple of kSlabAlign = 128 rows
static inline RowMap make_rowmap(int tokens, int n, int group) {
  RowMap r{tokens, 0, 0};
  if (group > 0 && group < n) { r.group = group; r.mpad = ceil_to(group * tokens, kSlabAlign); }
  return r;
}
static inline long total_rows(const RowMap& r, int n) {
  if (r.group <= 0) return (long)n * r.tokens;
  const int full = n / r.group, rest = n - full * r.group;
  return rest ? (long)full * r.mpad + (long)rest * r.tokens : (long)(full - 1) * r.mpad + (long)r.group * r.tokens;
}

// fp32 -> bf16 bits, round-to-nearest-even, NaN kept quiet (matches torch .to(bfloat16))
static inline uint16_t f2bf(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
static inline float bf2f(uint16_t b) {
  uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// ------------------------------------------------------------------------------------------------ engine
struct Mat {            // bf16 weight matrix [rows_pad, ld] zero padded
  uint8_t* w8 = nullptr;  // fp8 mode: e4m3 image [rows_pad, ld8] + one dequantisation scale per row (ssp2_set_precision)
  float* wscale = nullptr;
  int ld8 = 0, ld8_cap = 0;
  bf16* w = nullptr;
  float* b = nullptr;   // [rows_pad] fp32 holding bf16-rounded values
  int rows = 0, rows_pad = 0, cols = 0, ld = 0;
  bool w_set = false, b_set = false;
};
struct Layer {
  float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
  bool ln_set[4] = {false, false, false, false};
  Mat qkv, proj, fc1, fc2;
  int d_int = 0, ld_int = 0;
  bool attn_dropped = false;   // ssp2_drop_attention: bypass for good
  float o8_scale = ATTN_OUT8_SCALE;   // fp8 mode: the attention output of this block is handed to the out-projection as e4m3(o * o8_scale)
  int* keep_dev = nullptr;     // ssp2_prune_ffn_into: the kept-neuron list on the device
  // LayerScale (ssp2_set_layer_scale): fp32 [dim] per residual branch, [0] attention (timm ls1), [1] MLP (ls2); a branch whose scale
  // was set runs EPI_RESID_LS, any other EPI_RESID.  The storage (2 x ceil256(dim) floats per block) comes out of ssp2_create's arena, so
  // that setting a scale inside a caller's prune bracket is one small copy: no allocation, no memset
  float* ls[2] = {nullptr, nullptr};
  bool ls_set[2] = {false, false};
};
// the residual epilogue of block L's branch (0 attention, 1 MLP): with its LayerScale when one was set
static inline int resid_epi(const Layer& L, int branch, GemmArgs& g) {
  if (!L.ls_set[branch]) return EPI_RESID;
  g.ls = L.ls[branch];
  return EPI_RESID_LS;
}
// everything a block's attention half / MLP half reads has been loaded (the block loop and the tail ask before they launch)
static inline bool attn_loaded(const Layer& L) { return L.ln_set[0] && L.ln_set[1] && L.qkv.w_set && L.qkv.b_set && L.proj.w_set && L.proj.b_set; }
static inline bool mlp_loaded(const Layer& L) { return L.ln_set[2] && L.ln_set[3] && L.fc1.w_set && L.fc1.b_set && L.fc2.w_set && L.fc2.b_set; }

struct ssp2_engine {
  ssp2_vit_desc d{};
  std::vector<int32_t> d_int;
  int tokens = 0, patches = 0, side = 0, dh = 0;
  // token layout (ssp2_create_ext): prefix tokens in front of the patches (1: CLS; 2: CLS + distillation token) and whether the
  // logits average the CLS head with a distillation head on row 1 (tail_rows = rows the evaluation tail carries: 2 with it, else 1)
  int prefix = 1, dist_head = 0, tail_rows = 1;
  // (ssp2_create_layout) register tokens between CLS and the patches (prefix = 1 + reg_tokens; the head still reads row 0: tail_rows 1)
  // and whether pos carries the prefix tokens' rows (1: tokens rows) or the patches' only (0: class-free positions, timm no_embed_class)
  int reg_tokens = 0, pos_prefix_rows = 1;
  int kpe = 0, kpe_pad = 0, ld_int_max = 0;
  long rows_cap = 0;        // token-matrix rows the workspace is sized for
  hipStream_t stream = nullptr;
  int n_cu = 256;
  int dev = 0;             // HIP device the engine was created on
  int zig = 0;             // direction of the next large launch (next_dir)
  int zig_hold = -1;       // >= 0: the launches of a split operation all take this direction (next_dir does not advance)
  // Run-time switches (ssp2_set_option).  Their defaults are read from the environment ONCE, in ssp2_create (round 2 called
  // getenv on every launch); tests and A/B scripts flip them per handle.
  int opt[SSP2_OPT_END] = {};
  std::vector<void*> allocs;
  int arena_mode = 0;                       // ssp2_create: 1 = measuring pass, 2 = assigning pass (dalloc)
  size_t arena_need[2] = {0, 0};            // [0] zero-initialised, [1] written before read
  char* arena_cur[2] = {nullptr, nullptr};
  size_t ws_bytes = 0, weight_bytes = 0;

  Mat patch, head, head_dist;
  float *cls = nullptr, *pos = nullptr, *lnf_g = nullptr, *lnf_b = nullptr, *dist = nullptr;
  float* reg = nullptr;     // register tokens, fp32 [reg_tokens, dim] as loaded (ssp2_set_reg_tokens)
  bool misc_set[4] = {false, false, false, false};
  bool dist_set = false, reg_set = false;
  size_t pos_rows() const { return (size_t)(pos_prefix_rows ? tokens : patches); }      // rows of SSP2_T_POS
  std::vector<Layer> layers;

  // workspace (sized for max_images)
  bf16 *a_pe = nullptr, *hbuf = nullptr, *qkvbuf = nullptr, *obuf = nullptr, *actbuf = nullptr, *cls_h = nullptr;
  bf16* prebuf = nullptr;   // pre-GELU copy, only for models with < 128 tokens (unfused scoring)
  // evaluation tail (last block on the prefix rows only: tail_rows per image, prefix-major [tail_rows][n][...])
  float* x_cls = nullptr;
  bf16 *q_cls = nullptr, *o_cls = nullptr, *h_cls = nullptr, *act_cls = nullptr;
  float *slab = nullptr, *norms = nullptr, *logits = nullptr;

  bool fp8 = false;             // ssp2_set_precision(SSP2_PREC_FP8): QKV / fc1 / fc2 of launches with >= 4096 rows on e4m3 MFMA
  uint8_t *hbuf8 = nullptr, *act8 = nullptr;   // LayerNorm output / FFN activation as e4m3 bytes
  float* hscale = nullptr;                     // per-row activation scale of hbuf8 (amax / 448, written by the LayerNorm)
  unsigned int* ln_sync = nullptr;             // fused LayerNorm: queue heads + panel arrival counters (GemmArgs.ln_sync)
  unsigned int* dg_scratch = nullptr;          // deferred residual: 128 KiB per CU where a workgroup parks a tile (GemmArgs.dg)
  int ln_set = 0;                              // queue-head set of the next fused launch (the launch zeroes the other one)
  int n_xcc_seen = 0;
  bool xcc_ok = false;                         // XCC_ID probe at create: ids 0..7 seen, nothing else (else the fused form stays off)
  unsigned int* fp8_sat = nullptr;             // device counter of clipped e4m3 casts (SSP2_Q_FP8_SATURATED)
  unsigned long long* act8_top = nullptr;      // fp8 calibration: e4m3 bytes of the fc1 -> fc2 hand-off found ON the top code (SSP2_Q_FP8_FC2_TOP_CODES)
  unsigned int* attn_amax = nullptr;           // fp8 calibration: [depth] float bits of max |attention output| per block (ssp2_fp8_calibrate_*)
  bool fp8_calibrating = false;
  uint8_t* obuf8 = nullptr;                    // attention output as e4m3(o * 16) bytes: the A operand of the fp8 out-projection (SSP2_OPT_FP8_PROJ)
  int o_ld = 0;                                // row stride of obuf / o_cls in elements (0: dim, what the forward uses; ssp2_attention_bf16 sets it)
  int ld8_dim = 0, ld8_int_max = 0;
  float* stage_f32 = nullptr;   // staging buffer of ssp2_load_tensor (host sources)
  size_t stage_cap = 0;

  // ssp2_prune_ffn scratch (allocated at the first call, sized for the widest block: later calls allocate nothing)
  bf16 *prune_t1 = nullptr, *prune_t2 = nullptr;
  float* prune_tb = nullptr;
  int* prune_keep = nullptr;
  size_t prune_t1_cap = 0, prune_t2_cap = 0, prune_tb_cap = 0, prune_keep_cap = 0;

  // keep lists of ssp2_prune_ffn / ssp2_prune_ffn_into cross PCIe out of an ENGINE-OWNED pinned buffer, one slot per layer
  // (stage_keep): the caller's list may be pinned memory itself, and a copy out of pinned memory is truly asynchronous
  int32_t* keep_pin = nullptr;
  size_t keep_pin_slot = 0;
  std::vector<hipEvent_t> keep_ev;
  std::vector<char> keep_ev_set;

  // profiling: prof_class = one SSP2_K_* class, SSP2_K_COUNT = every class, -1 = off
  int prof_class = -1;
  struct ProfEvent { hipEvent_t a, b; int klass; };
  std::vector<ProfEvent> prof_events;
  double prof_flops[SSP2_K_COUNT] = {};   // algorithmic flops of the recorded launches (2*M*N*K; attention: 4*N*N*d_h per head and image)
  double prof_bytes[SSP2_K_COUNT] = {};   // algorithmic HBM bytes of the recorded launches (the memory-bound classes)
};

// hipFuncSetAttribute state is per DEVICE (round 2 kept one flag per process: wrong the moment one process drives two GPUs)
static const int kMaxDevices = 64;
static inline int cur_device() { int d = 0; return (hipGetDevice(&d) == hipSuccess && d >= 0 && d < kMaxDevices) ? d : 0; }

// ssp2_create runs its allocation sequence TWICE: a measuring pass (arena_mode 1: sizes only), then ONE hipMalloc + ONE hipMemset for
// everything that must start as zeros and ONE hipMalloc for the buffers that are always written before they are read (qkv, FFN activation:
// 8 of the 10.5 GB of a layer-major ViT-B/16 workspace), then the assigning pass (arena_mode 2).  Rounds 1-4 issued ~250 hipMalloc + 250
// synchronous hipMemset per engine and zeroed all of it: 4 ms of every prune through the reference-named API, whose engine is built
// inside the prune bracket.  Outside ssp2_create (arena_mode 0: fp8 weight images, on-demand buffers) every buffer is its own allocation.
template <typename T>
static int dalloc(ssp2_engine* e, T** p, size_t count, bool workspace, bool zero = true) {
  void* q = nullptr;
  size_t bytes = count * sizeof(T);
  if (bytes == 0) bytes = 16;
  if (e->arena_mode == 1) {
    e->arena_need[zero ? 0 : 1] += (bytes + 255) & ~(size_t)255;
    *p = nullptr;
    return 0;
  }
  if (e->arena_mode == 2) {
    char*& cur = e->arena_cur[zero ? 0 : 1];
    *p = (T*)cur;
    cur += (bytes + 255) & ~(size_t)255;
    (workspace ? e->ws_bytes : e->weight_bytes) += bytes;
    return 0;
  }
  if (hipMalloc(&q, bytes) != hipSuccess) return fail(SSP2_ENOMEM, "hipMalloc(%zu) failed", bytes);
  if (zero && hipMemset(q, 0, bytes) != hipSuccess) return fail(SSP2_EHIP, "hipMemset failed");
  e->allocs.push_back(q);
  (workspace ? e->ws_bytes : e->weight_bytes) += bytes;
  *p = (T*)q;
  return 0;
}

static int mat_alloc(ssp2_engine* e, Mat& m, int rows, int cols) {
  m.rows = rows; m.cols = cols;
  m.rows_pad = ceil_to(rows, 256);   // a multiple of both kernels' BN (128 / 256)
  m.ld = ceil_to(cols, GEMM_BK);
  int rc;
  if ((rc = dalloc(e, &m.w, (size_t)m.rows_pad * m.ld, false))) return rc;
  if ((rc = dalloc(e, &m.b, (size_t)m.rows_pad, false))) return rc;
  return 0;
}

// Zigzag launch order: every large launch (persistent GEMM, LayerNorm, persistent attention) walks its row panels in the
// direction opposite to the previous launch's, so it starts on the rows its producer wrote LAST — the ones still in the
// 256 MiB Infinity Cache — instead of on the oldest, which its own traffic would evict before it gets to the fresh ones
// (the streaming pathology of an LRU cache smaller than the tensor: 194 MB of x, 290 MB of qkv, 387 MB of activations per
// 320 images).  Results do not depend on the order.  Same-box A/B, three boxes: -0.8 % of the step
// (profiles/r02_f_zigzag_ab.txt); SSP2_ZIGZAG=0 switches it off.
static int next_dir(ssp2_engine* e) {
  if (!e->opt[SSP2_OPT_ZIGZAG]) return 0;
  if (e->zig_hold >= 0) return e->zig_hold;
  const int d = e->zig; e->zig ^= 1; return d;
}

struct ProfScope {
  ssp2_engine* e; bool on; int klass; hipEvent_t a{}, b{};
  ProfScope(ssp2_engine* e_, int klass_, double flops = 0, double bytes = 0)
      : e(e_), on(klass_ >= 0 && klass_ < SSP2_K_COUNT && (e_->prof_class == klass_ || e_->prof_class == SSP2_K_COUNT)), klass(klass_) {
    if (on) { hipEventCreate(&a); hipEventCreate(&b); hipEventRecord(a, e->stream); e->prof_flops[klass] += flops; e->prof_bytes[klass] += bytes; }
  }
  ~ProfScope() {
    if (on) { hipEventRecord(b, e->stream); e->prof_events.push_back({a, b, klass}); }
  }
};

// ------------------------------------------------------------------------------------------------ launches
// Large-M projections go to the 256 x 256 tile kernel (bit-identical results, fewer LDS-DMA issues per MFMA);
// everything else (small M, fused fc1 epilogue, patch embed, head) stays on the 128 x 128 kernel.
static const int kBigTileMinRowsDefault = 4096;   // SSP2_OPT_BIG_TILE_MIN_ROWS
static inline int big_tile_min_rows(const ssp2_engine* e) { return e->opt[SSP2_OPT_BIG_TILE_MIN_ROWS]; }
template <int EPI, int SCORE = 0, bool F8 = false>
static int launch_gemm256(ssp2_engine* e, GemmArgs g, int klass) {
  g.tiles_m = (g.M + 255) / 256;
  g.tiles_n = (g.N + 255) / 256;
  // tile order: plain N-fastest unless SSP2_OPT_GROUP256 asks for column groups (100 * GM + GN, see gemm256.hip.h set_tile)
  g.group_m = (EPI == EPI_RESID && SCORE >= 3) ? 0 : e->opt[SSP2_OPT_GROUP256];
  if (F8 && (g.K % 128 || !g.wscale)) return fail(SSP2_EINVAL, "fp8 GEMM needs K %% 128 == 0 and per-row weight scales (K=%d)", g.K);
  static bool attr_done[kMaxDevices] = {};
  if (!attr_done[e->dev]) {
    HIPCHK(hipFuncSetAttribute((const void*)gemm256_entry<EPI, SCORE, F8>(), hipFuncAttributeMaxDynamicSharedMemorySize, G256::LDS));
    attr_done[e->dev] = true;
  }
  g.nt_out = e->opt[SSP2_OPT_NT_STORES];
  if (!(EPI == EPI_RESID && SCORE >= 3)) g.reverse = next_dir(e);
  else { g.ln_sync = e->ln_sync; g.ln_set = e->ln_set; e->ln_set ^= 1; }      // LayerNorm behind the epilogue: per-XCD tile queues
  if (EPI == EPI_RESID && SCORE == 1) {
    if (!e->dg_scratch || g.N % 256 || g.K / 64 < 4) return fail(SSP2_EINVAL, "deferred residual: N %% 256, K >= 256 and the parking area are required");
    g.dg = e->dg_scratch;
  }
  ProfScope ps(e, klass, 2.0 * g.M * (double)g.N * g.K);
  const int wgs = std::min(g.tiles_m * g.tiles_n, e->n_cu);
  hipLaunchKernelGGL((gemm256_entry<EPI, SCORE, F8>()), dim3(wgs), dim3(512), G256::LDS, e->stream, g);
  HIPCHK(hipGetLastError());
  return 0;
}

// The residual projections (attention out-proj, fc2) can normalise the rows they finish — the LayerNorm that feeds the
// NEXT projection — inside the GEMM kernel (gemm256.hip.h, LNV): the standalone kernel (4.5 KB per row through HBM, 9 % of
// the step) then does not run for that LayerNorm.  OPT-IN (SSP2_LN_FUSION=1 / ssp2_set_option; 2 = the same, kept for the tests
// that ask for "always"), because neither form built so far pays:
//   round 2  one workgroup owns a whole 256-row panel and walks its dim / 256 column tiles one after the other: the A panel is
//            read that many times from the Infinity Cache (profiles/r02_d_gemm_ln_fusion.txt);
//   round 3  VERDICT r02's form: plain tile order, per-XCD work queues keyed on the hardware's XCC_ID, and the panel's
//            LAST-ARRIVING workgroup normalises it — no spin-wait, no extra barrier, one returning atomic per tile hidden behind
//            the epilogue.  The scheduling is free (queues + arrivals without the LayerNorm phase time like the plain kernel,
//            +-1 %), and the phase costs EXACTLY what the standalone launch costs: 499 us for 630 400 rows inside out-proj
//            against 490 us alone, 257 against 245 us for 315 200 rows inside fc2 (profiles/r03_q_ln_fusion_last_arriver.txt) —
//            with two, four or eight rows in flight per wave and with the rows' dependent chains interleaved in pairs alike.
//            The panel's rows are not in the L2 any more when its last tile is done (the XCD's 32 CUs write 8 MB per tile round
//            into 4 MB), so the phase reads them back through the same saturated memory system as the standalone kernel, from a
//            CU whose matrix pipe idles meanwhile: the same bytes at the same 5.7 TB/s, now on the GEMM's critical path.  Step
//            A/B: +0.6 % (slower).  A fusion that pays would have to keep the finished rows ON the CU (registers / LDS) until the
//            whole row exists — a 256 x dim fp32 panel per workgroup, which the 256 x 256 tile's accumulators leave no room for.
// Results are bit-identical either way (one row routine, ln_row_finish; tests/test_gpu_parity.py).
// Conditions when switched on: the launch goes to the 256 x 256 kernel, dim = 3, 4 or 5 column tiles, at least two K-tiles per
// tile (the tile stream), and the XCC_ID probe at create saw nothing but ids 0..7.  Returns dim / 256 or 0.
static int ln_fusable(const ssp2_engine* e, int M, int K, bool f8) {
#ifndef SSP2_LAB
  return 0;               // product build: the fused form is not instantiated (lab build: lib/libssp2vit_lab.so)
#endif
  const int D = e->d.dim;
  const int on = e->opt[SSP2_OPT_LN_FUSION];
  if (!on || !e->xcc_ok || M < big_tile_min_rows(e) || D % 256 || D / 256 < 3 || D / 256 > 5 || !e->opt[SSP2_OPT_BIG_TILES]) return 0;
  if (K / (f8 ? 128 : 64) < 2) return 0;
  // The kernel keeps EIGHT tile queues, one per XCC_ID, and a queue is drained only by workgroups that run on that XCD: all eight
  // ids must have been seen by the probe (a CPX / DPX partition shows fewer), and the launch must be wide enough that the
  // dispatcher's round-robin puts workgroups on every XCD — at least 8 per XCD here, which ssp2_set_cu_limit(h, n < 64) or a
  // launch of fewer than 64 tiles does not give.  Otherwise the standalone LayerNorm runs (same bits).
  const long tiles = (long)((M + 255) / 256) * (D / 256);
  if (e->n_xcc_seen != 8 || std::min<long>(tiles, e->n_cu) < 64) return 0;
  return D / 256;
}
template <bool F8>
static int launch_resid_ln(ssp2_engine* e, const GemmArgs& g, int lnv, int klass) {
#ifdef SSP2_LAB
  switch (lnv) {
    case 3: return launch_gemm256<EPI_RESID, 3, F8>(e, g, klass);
    case 4: return launch_gemm256<EPI_RESID, 4, F8>(e, g, klass);
    case 5: return launch_gemm256<EPI_RESID, 5, F8>(e, g, klass);
    default: return fail(SSP2_EINVAL, "fused LayerNorm: dim / 256 = %d unsupported", lnv);
  }
#else
  return fail(SSP2_ESTATE, "fused LayerNorm (dim / 256 = %d) exists in the lab build only", lnv);
#endif
}

template <int EPI, int SCORE = 0>
static int launch_gemm_small(ssp2_engine* e, GemmArgs g, int klass);
template <int EPI, int SCORE = 0>
static int launch_gemm(ssp2_engine* e, GemmArgs g, int klass) {
  if (g.K % GEMM_BK) return fail(SSP2_EINVAL, "GEMM K=%d not a multiple of %d", g.K, GEMM_BK);
  if constexpr (EPI == EPI_BF16 || EPI == EPI_RESID || EPI == EPI_RESID_LS || EPI == EPI_FC1) {
    if (g.M >= big_tile_min_rows(e) && !(EPI == EPI_FC1 && (g.out2 || !e->opt[SSP2_OPT_FC1_BIG_TILES])) && e->opt[SSP2_OPT_BIG_TILES]) {
#ifdef SSP2_LAB
      if constexpr (EPI == EPI_RESID && SCORE == 0) {      // the deferred residual (same bits): full column tiles, a main loop long enough to ride on
        if (e->opt[SSP2_OPT_DEFER_RESID] && e->dg_scratch && g.N % 256 == 0 && g.K / 64 >= 4) return launch_gemm256<EPI_RESID, 1>(e, g, klass);
      }
#endif
      return launch_gemm256<EPI, SCORE>(e, g, klass);
    }
  }
  return launch_gemm_small<EPI, SCORE>(e, g, klass);
}
template <int EPI, int SCORE>
static int launch_gemm_small(ssp2_engine* e, GemmArgs g, int klass) {
  g.tiles_m = (g.M + GEMM_BM - 1) / GEMM_BM;
  if (g.tiles_m <= 0 || g.tiles_n <= 0) return fail(SSP2_EINVAL, "empty GEMM");
  static bool attr_done[kMaxDevices] = {};
  if (!attr_done[e->dev]) {
    HIPCHK(hipFuncSetAttribute((const void*)gemm_bf16_kernel<EPI, SCORE>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_BYTES));
    attr_done[e->dev] = true;
  }
  ProfScope ps(e, klass, 2.0 * g.M * (double)g.N * g.K);
  hipLaunchKernelGGL((gemm_bf16_kernel<EPI, SCORE>), dim3(g.tiles_m * g.tiles_n), dim3(256), GEMM_LDS_BYTES, e->stream, g);
  HIPCHK(hipGetLastError());
  return 0;
}

// How a weight matrix and an activation become the operand half of a launch: A, lda, W, ldw, bias, K, the e4m3 scales, M, N and
// tiles_n.  What else a launch needs (out / ldo, x / xin / ldx, the scoring and fused-LayerNorm fields, out2, group_m) is set where it
// is launched.  The kernels take e4m3 operands through the bf16 pointers of GemmArgs, with lda / ldw / K / ldo counting BYTES: those
// casts, and the byte-versus-element row arithmetic they bring (gemm_rows_from), are written here and nowhere else.
struct ActOperand {        // the A operand: bf16 rows (p, ld in elements) or e4m3 bytes (p8, ld in bytes) with their dequantisation
  const bf16* p; const uint8_t* p8; int ld;
  const float* scale; float scale_const;     // e4m3: one scale per row, or (scale == nullptr) one for the whole operand (0 = 1)
};
static inline ActOperand act_bf16(const bf16* p, int ld) { return ActOperand{p, nullptr, ld, nullptr, 0.f}; }
static inline ActOperand act_e4m3(const uint8_t* p8, int ld, const float* scale, float scale_const = 0.f) { return ActOperand{nullptr, p8, ld, scale, scale_const}; }
// ... against caller-owned weight rows (the operator entries): w_dev is bf16, or e4m3 bytes when the activation is
static GemmArgs gemm_operands(const ActOperand& a, const void* w_dev, int ldw, const float* wscale, const float* bias, int M, int N, int K, int tiles_n) {
  GemmArgs g{};
  g.A = a.p8 ? (const bf16*)a.p8 : a.p; g.lda = a.ld; g.W = (const bf16*)w_dev; g.ldw = ldw; g.bias = bias;
  g.M = M; g.N = N; g.K = K; g.tiles_n = tiles_n;       // (tiles_n: column tiles of the 128 x 128 kernel; the 256 x 256 launch counts its own)
  if (a.p8) { g.wscale = wscale; g.ascale = a.scale; g.ascale_const = a.scale_const; }
  return g;
}
// ... against an engine matrix, in the activation's format: K is the matrix's padded row length in that format, N the columns the
// launch stores.  (An e4m3 activation against a matrix ssp2_set_precision has not quantised leaves wscale null: the fp8 launch refuses it.)
static GemmArgs bind(const Mat& m, const ActOperand& a, int M, int N) {
  return a.p8 ? gemm_operands(a, m.w8, m.ld8, m.wscale, m.b, M, N, m.ld8, m.rows_pad / GEMM_BN)
              : gemm_operands(a, m.w, m.ld, nullptr, m.b, M, N, m.ld, m.rows_pad / GEMM_BN);
}
static inline bool has_e4m3(const Mat& m) { return m.w8 != nullptr; }      // ssp2_set_precision has quantised it
// ... against the N weight rows from row0 on (bf16): the evaluation tail's query and key / value slices of qkv
static GemmArgs bind_rows(const Mat& m, int row0, const ActOperand& a, int M, int N) {
  GemmArgs g = bind(m, a, M, N);
  g.W += (size_t)row0 * m.ld; g.bias += row0; g.tiles_n = (N + GEMM_BN - 1) / GEMM_BN;
  return g;
}
// rows [row0, M) of an fc1 launch (the second launch of the prefix split): operand, per-row scales and output move on by row0 rows,
// whose elements are bytes for the fp8 fc1 (e4m3 in, e4m3 out) and bf16 otherwise
static GemmArgs gemm_rows_from(const GemmArgs& g, int row0) {
  GemmArgs r = g;
  const size_t esz = g.wscale ? 1 : sizeof(bf16);
  r.M = g.M - row0; r.ascale = g.ascale ? g.ascale + row0 : nullptr;
  r.A = (const bf16*)((const uint8_t*)g.A + (size_t)row0 * g.lda * esz); r.out = (bf16*)((uint8_t*)g.out + (size_t)row0 * g.ldo * esz);
  return r;
}

// The one table from what a launch is at run time — epilogue, score site (g.score_site), operand format, and the width lnv = dim / 256
// of a LayerNorm fused behind a residual epilogue (ln_fusable; 0 = none) — to the template instantiation that runs it.  bf16 operands go
// through launch_gemm's choice of tile, e4m3 operands have the 256 x 256 kernel only.  The forms listed are the ones the library
// launches: anything else is refused, not instantiated (tests/test_host_cpu.py counts the gemm256 forms of the product build).
static_assert(SSP2_EPI_BF16 == EPI_BF16 && SSP2_EPI_RESID == EPI_RESID && SSP2_EPI_GELU == EPI_FC1, "the operator entries pass their epilogue code on as it is");
static int dispatch_gemm(ssp2_engine* e, int epi, bool f8, const GemmArgs& g, int klass, int lnv = 0) {
  const int site = g.score_site;
#define GEMM_FORM(EPI_, SITE_) (f8 ? launch_gemm256<EPI_, SITE_, true>(e, g, klass) : launch_gemm<EPI_, SITE_>(e, g, klass))
  if (epi == EPI_BF16 && !site && !lnv) return GEMM_FORM(EPI_BF16, 0);
  if (epi == EPI_RESID && !site && lnv) return f8 ? launch_resid_ln<true>(e, g, lnv, klass) : launch_resid_ln<false>(e, g, lnv, klass);
  if (epi == EPI_RESID && !site) return GEMM_FORM(EPI_RESID, 0);
  if (epi == EPI_RESID_LS && !site && !lnv && g.ls) return GEMM_FORM(EPI_RESID_LS, 0);     // (no lab form behind it: see attn_half / mlp_half)
  if (epi == EPI_FC1 && !lnv && site == 1) return GEMM_FORM(EPI_FC1, 1);
  if (epi == EPI_FC1 && !lnv && site == 2) return GEMM_FORM(EPI_FC1, 2);
  if (epi == EPI_FC1 && !lnv && site == 0) return GEMM_FORM(EPI_FC1, 0);
#undef GEMM_FORM
  return fail(SSP2_EINVAL, "no GEMM kernel for epilogue %d with score site %d, %s operands, fused LayerNorm width %d", epi, site, f8 ? "e4m3" : "bf16", lnv);
}

static int launch_ln(ssp2_engine* e, const float* x, size_t in_stride, const float* g, const float* b, bf16* y,
                     int out_ld, int rows, int D, RowMap gather = RowMap{0, 0, 0}, uint8_t* y8 = nullptr, float* ascale = nullptr) {
  ProfScope ps(e, SSP2_K_LN, 0, (double)rows * D * (4.0 + (y8 ? 1.0 : 2.0)));     // fp32 row in, bf16 / e4m3 row out
  dim3 grid((rows + 3) / 4), blk(256);
  // one instantiation per row width in 256-element steps: the row lives in MAXV float4 registers per lane, and a
  // wider instantiation than needed drags predicated dead chunks along (ViT-L/16 on <8>: 3.1 TB/s; on <4>: see DESIGN)
  const int rev = rows >= big_tile_min_rows(e) ? next_dir(e) : 0;
#define LN_CASE(V) do { if (D == 256 * V) hipLaunchKernelGGL((layernorm_bf16_kernel<V, true>), grid, blk, 0, e->stream, x, in_stride, g, b, y, out_ld, rows, D, e->d.ln_eps, gather, y8, rev, ascale); \
                        else hipLaunchKernelGGL((layernorm_bf16_kernel<V, false>), grid, blk, 0, e->stream, x, in_stride, g, b, y, out_ld, rows, D, e->d.ln_eps, gather, y8, rev, ascale); } while (0)
  if (D <= 256 * 1) LN_CASE(1);
  else if (D <= 256 * 2) LN_CASE(2);
  else if (D <= 256 * 3) LN_CASE(3);
  else if (D <= 256 * 4) LN_CASE(4);
  else if (D <= 256 * 5) LN_CASE(5);
  else if (D <= 256 * 8) LN_CASE(8);
#undef LN_CASE
  else
    return fail(SSP2_EINVAL, "LayerNorm width %d > 2048 unsupported", D);
  HIPCHK(hipGetLastError());
  return 0;
}

template <int DH, int NT, bool CLS>
static int launch_attn_t(ssp2_engine* e, int n, RowMap rm, uint8_t* out8 = nullptr, float out8_scale = ATTN_OUT8_SCALE) {
  // d_h = 64: 128-byte K and V rows (LDS-DMA staging) + 4 KiB per wave of output staging; else padded rows
  // d_h = 80 with a whole number of 1-KiB DMA pieces: 160-byte rows + 64 bytes of slack behind V (attn.hip.h)
  constexpr int smem = DH == 64 ? NT * 32 * 256 + 4 * 4096
                     : (DH == 80 && (NT * 32 * 10) % 64 == 0) ? NT * 32 * 320 + 64
                     : NT * 32 * (DH * 2 + 16) + NT * 32 * 192;
  static bool attr_done[kMaxDevices] = {};
  if (!attr_done[e->dev]) {
    HIPCHK(hipFuncSetAttribute((const void*)attn_fwd_kernel<DH, NT, CLS>, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    attr_done[e->dev] = true;
  }
  const int D = e->d.dim, ld = 3 * D, ldo = e->o_ld > 0 ? e->o_ld : D;
  // algorithmic work of a full attention: S = QK^T and O = PV, 2 * N * N * d_h flops each per (image, head); q, k, v read, o written
  const double qn = CLS ? (double)e->tail_rows : (double)e->tokens;
  ProfScope ps(e, SSP2_K_ATTN, 4.0 * qn * e->tokens * DH * e->d.heads * n, 2.0 * n * D * (2.0 * e->tokens + 2.0 * qn));
  if constexpr (DH == 64 && !CLS && NT >= 4 && NT <= 7) {
    // persistent producer / consumer form (attn.hip.h); SSP2_OPT_ATTN_PERSIST = 0 keeps the one-item-per-workgroup kernel
    if (e->opt[SSP2_OPT_ATTN_PERSIST]) {
      constexpr int psmem = 2 * 2 * NT * 32 * 128 + 7 * 4096;
      static bool pattr_done[kMaxDevices] = {};
      if (!pattr_done[e->dev]) {
        HIPCHK(hipFuncSetAttribute((const void*)attn64_persist_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, psmem));
        pattr_done[e->dev] = true;
      }
      const long items = (long)e->d.heads * n;
      if (items > 0x7fffffffL) return fail(SSP2_EINVAL, "too many attention items");
      const int rev = next_dir(e);
      // 197 tokens (every /16 model at 224 pixels): five valid keys in the seventh key tile = ONE live register group — the instantiation that
      // knows it at compile time emits no maxima / exponentials / sums for the other three groups and no P V step for the dead half (attn.hip.h LIVE)
      if (NT == 7 && (e->tokens - 32 * (NT - 1) + 7) >> 3 == 1 && e->opt[SSP2_OPT_ATTN_LIVE]) {
        static bool lattr_done[kMaxDevices] = {};
        if (!lattr_done[e->dev]) {
          HIPCHK(hipFuncSetAttribute((const void*)attn64_persist_kernel<NT, (NT == 7 ? 1 : 0)>, hipFuncAttributeMaxDynamicSharedMemorySize, psmem));
          lattr_done[e->dev] = true;
        }
        hipLaunchKernelGGL((attn64_persist_kernel<NT, (NT == 7 ? 1 : 0)>), dim3((unsigned)std::min<long>(items, e->n_cu)), dim3(512), psmem, e->stream, e->qkvbuf, ld,
                           e->obuf, ldo, e->tokens, D, e->d.heads, (int)items, 1.0f / sqrtf((float)DH), rm, rev, e->opt[SSP2_OPT_ATTN_STAGGER], out8, e->ld8_dim, e->fp8_sat, out8_scale);
      } else
      hipLaunchKernelGGL((attn64_persist_kernel<NT>), dim3((unsigned)std::min<long>(items, e->n_cu)), dim3(512), psmem, e->stream, e->qkvbuf, ld,
                         e->obuf, ldo, e->tokens, D, e->d.heads, (int)items, 1.0f / sqrtf((float)DH), rm, rev, e->opt[SSP2_OPT_ATTN_STAGGER], out8, e->ld8_dim, e->fp8_sat, out8_scale);
      HIPCHK(hipGetLastError());
      return 0;
    }
  }
  if constexpr (DH == 80 && !CLS && NT == 9) {
    // persistent form for d_h = 80 (ViT-H/14): two K buffers + one V buffer, every wave consumer and DMA issuer (attn.hip.h);
    // its ninth query tile must hold exactly one query (257 tokens), which it splits over the waves by key tile
    if (e->opt[SSP2_OPT_ATTN_PERSIST] && e->tokens == 32 * (NT - 1) + 1) {
      constexpr int psmem = 3 * NT * 32 * 160 + 64 + 1024 + 8 * 96 * 4;      // K ring + V + slack + the split ninth tile's query row and partials (attn.hip.h)
      static bool pattr_done[kMaxDevices] = {};
      if (!pattr_done[e->dev]) {
        HIPCHK(hipFuncSetAttribute((const void*)attn80_persist_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, psmem));
        pattr_done[e->dev] = true;
      }
      const long items = (long)e->d.heads * n;
      if (items > 0x7fffffffL) return fail(SSP2_EINVAL, "too many attention items");
      const int rev = next_dir(e);
      // 257 tokens: ONE valid key in the ninth key tile = one live register group, known at compile time (attn.hip.h LIVE)
      if (e->opt[SSP2_OPT_ATTN_LIVE]) {
        static bool lattr_done[kMaxDevices] = {};
        if (!lattr_done[e->dev]) {
          HIPCHK(hipFuncSetAttribute((const void*)attn80_persist_kernel<NT, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, psmem));
          lattr_done[e->dev] = true;
        }
        hipLaunchKernelGGL((attn80_persist_kernel<NT, 1>), dim3((unsigned)std::min<long>(items, e->n_cu)), dim3(512), psmem, e->stream, e->qkvbuf, ld,
                           e->obuf, ldo, e->tokens, D, e->d.heads, (int)items, 1.0f / sqrtf((float)DH), rm, rev, e->opt[SSP2_OPT_ATTN_STAGGER], out8, e->ld8_dim, e->fp8_sat, out8_scale);
      } else
      hipLaunchKernelGGL((attn80_persist_kernel<NT>), dim3((unsigned)std::min<long>(items, e->n_cu)), dim3(512), psmem, e->stream, e->qkvbuf, ld,
                         e->obuf, ldo, e->tokens, D, e->d.heads, (int)items, 1.0f / sqrtf((float)DH), rm, rev, e->opt[SSP2_OPT_ATTN_STAGGER], out8, e->ld8_dim, e->fp8_sat, out8_scale);
      HIPCHK(hipGetLastError());
      return 0;
    }
  }
  if (out8) return fail(SSP2_ESTATE, "e4m3 attention output needs a persistent attention kernel (d_h = 64 / 80, SSP2_OPT_ATTN_PERSIST)");
  if (CLS)   // q from the compact prefix-major [tail_rows][n, D] projection, rows < tail_rows kept, output in the same order
    hipLaunchKernelGGL((attn_fwd_kernel<DH, NT, true>), dim3(e->d.heads, n), dim3(256), smem, e->stream, e->qkvbuf, ld, e->q_cls,
                       (size_t)D, n * D, e->o_cls, (size_t)ldo, n * ldo, e->tokens, D, 1.0f / sqrtf((float)DH), rm, e->tail_rows);
  else
    hipLaunchKernelGGL((attn_fwd_kernel<DH, NT, false>), dim3(e->d.heads, n), dim3(256), smem, e->stream, e->qkvbuf, ld, e->qkvbuf,
                       (size_t)e->tokens * ld, ld, e->obuf, (size_t)e->tokens * ldo, ldo, e->tokens, D, 1.0f / sqrtf((float)DH), rm);
  HIPCHK(hipGetLastError());
  return 0;
}

static_assert(ATTN_STREAM_MAX_TOKENS == SSP2_ATTN_STREAM_MAX_TOKENS, "attn_stream.hip.h and ssp2vit.h state the same maximum");
// (head dim, 32-key tiles) pairs of the resident kernels (attn.hip.h): K, V and a query's score row fit LDS / registers
static bool attn_resident(int dh, int tokens) {
  const int nt = (tokens + 31) / 32;
  return (dh == 64 && nt >= 1 && nt <= 9) || (dh == 80 && nt == 9) || (dh == 16 && nt == 1);
}
static bool attn_stream_ok(int dh, int tokens) { return dh == 64 && tokens >= 1 && tokens <= ATTN_STREAM_MAX_TOKENS; }
// SSP2_OPT_ATTN_STREAM: 1 = sequences without a resident kernel stream, 2 = every d_h = 64 attention streams
static bool attn_streams(int mode, int dh, int tokens) {
  return attn_stream_ok(dh, tokens) && (mode >= 2 || (mode == 1 && !attn_resident(dh, tokens)));
}
// which geometries have a persistent kernel (they can write the e4m3 output); never the streaming route
static bool attn_persistent_for(int stream, int persist, int dh, int tokens) {
  const int nt = (tokens + 31) / 32;
  if (attn_streams(stream, dh, tokens)) return false;
  return persist && ((dh == 64 && nt >= 4 && nt <= 7) || (dh == 80 && nt == 9 && tokens == 257));
}
static bool attn_persistent(const ssp2_engine* e) { return attn_persistent_for(e->opt[SSP2_OPT_ATTN_STREAM], e->opt[SSP2_OPT_ATTN_PERSIST], e->dh, e->tokens); }
static bool attn_streaming(const ssp2_engine* e) { return attn_streams(e->opt[SSP2_OPT_ATTN_STREAM], e->dh, e->tokens); }
// "this engine's full attention can write e4m3": a persistent kernel, or the key-streaming kernel's OUT8 form (SSP2_OPT_STREAM_FP8)
static bool attn_writes_e4m3(const ssp2_engine* e) { return attn_persistent(e) || (attn_streaming(e) && e->opt[SSP2_OPT_STREAM_FP8]); }
// geometries launch_attn below has a kernel for under the streaming mode `stream` — checked when an engine is created, so that an
// unsupported geometry fails THERE and not at the first forward
static bool attn_supported(int dh, int tokens, int stream = 0) {
  return attn_resident(dh, tokens) || attn_streams(stream, dh, tokens);
}
// the key-streaming kernels (attn_stream.hip.h): full attention over the slab / dense rows, or the CLS-only tail
static int launch_attn_stream(ssp2_engine* e, int n, RowMap rm, bool cls_only, uint8_t* out8 = nullptr, float out8_scale = ATTN_OUT8_SCALE) {
  const int D = e->d.dim, ld = 3 * D, ldo = e->o_ld > 0 ? e->o_ld : D, T = e->tokens;
  const double qn = cls_only ? (double)e->tail_rows : (double)T;
  ProfScope ps(e, SSP2_K_ATTN, 4.0 * qn * T * 64 * e->d.heads * n, 2.0 * n * D * (2.0 * T + 2.0 * qn));
  const long items = (long)e->d.heads * n;
  const float scale = 1.0f / sqrtf(64.0f);
  if (cls_only) {
    if ((items + 3) / 4 > 0x7fffffffL) return fail(SSP2_EINVAL, "too many attention items");
    if (e->tail_rows == 2)   // CLS and DIST queries in one wave: shared key / value loads, two online-softmax states
      hipLaunchKernelGGL(attn64_stream_cls_kernel<2>, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, e->stream, e->qkvbuf, ld, e->q_cls, (size_t)D,
                         e->o_cls, (size_t)ldo, T, D, e->d.heads, (int)items, scale, rm, (size_t)n * D, (size_t)n * ldo);
    else
      hipLaunchKernelGGL(attn64_stream_cls_kernel<1>, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, e->stream, e->qkvbuf, ld, e->q_cls, (size_t)D,
                         e->o_cls, (size_t)ldo, T, D, e->d.heads, (int)items, scale, rm);
  } else {
    const int qblocks = (T + 32 * ATTN_STREAM_QW - 1) / (32 * ATTN_STREAM_QW);
    if (items * qblocks > 0x7fffffffL) return fail(SSP2_EINVAL, "too many attention items");
    static bool attr_done[2][kMaxDevices] = {};
    if (!attr_done[out8 != nullptr][e->dev]) {
      HIPCHK(hipFuncSetAttribute(out8 ? (const void*)attn64_stream_kernel<true> : (const void*)attn64_stream_kernel<false>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, ATTN_STREAM_SMEM));
      attr_done[out8 != nullptr][e->dev] = true;
    }
    if (out8)   // the e4m3 bytes of the fp8 out-projection's operand instead of the bf16 output (SSP2_OPT_STREAM_FP8)
      hipLaunchKernelGGL(attn64_stream_kernel<true>, dim3((unsigned)(items * qblocks)), dim3(64 * (ATTN_STREAM_QW + 1)), ATTN_STREAM_SMEM, e->stream,
                         e->qkvbuf, ld, (bf16*)nullptr, ldo, T, D, e->d.heads, qblocks, scale, rm, out8, e->ld8_dim, e->fp8_sat, out8_scale);
    else
      hipLaunchKernelGGL(attn64_stream_kernel<false>, dim3((unsigned)(items * qblocks)), dim3(64 * (ATTN_STREAM_QW + 1)), ATTN_STREAM_SMEM, e->stream,
                         e->qkvbuf, ld, e->obuf, ldo, T, D, e->d.heads, qblocks, scale, rm, (uint8_t*)nullptr, 0, (unsigned int*)nullptr, 0.f);
  }
  HIPCHK(hipGetLastError());
  return 0;
}
static int launch_attn(ssp2_engine* e, int n, RowMap rm, bool cls_only = false, uint8_t* out8 = nullptr, float out8_scale = ATTN_OUT8_SCALE) {
  if (attn_streaming(e)) {
    if (out8 && (cls_only || !e->opt[SSP2_OPT_STREAM_FP8])) return fail(SSP2_ESTATE, "the key-streaming attention writes bf16 only (no e4m3 output)");
    return launch_attn_stream(e, n, rm, cls_only, out8, out8_scale);
  }
  const int nt = (e->tokens + 31) / 32;
#define ATTN_CASE(DH_, NT_) if (e->dh == DH_ && nt == NT_) return cls_only ? launch_attn_t<DH_, NT_, true>(e, n, rm) : launch_attn_t<DH_, NT_, false>(e, n, rm, out8, out8_scale)
  ATTN_CASE(64, 7);   // 224/16: 197 tokens (Ti/S/B/L)
  ATTN_CASE(80, 9);   // 224/14: 257 tokens (H/14)
  ATTN_CASE(16, 1);   // reference smoke config: 32/16, 5 tokens
  ATTN_CASE(64, 1);
  ATTN_CASE(64, 2);   // 112/16: 50 tokens (test sizes)
  ATTN_CASE(64, 3);
  ATTN_CASE(64, 4);   // 160/16: 101 tokens
  ATTN_CASE(64, 5);   // 192/16: 145 tokens
  ATTN_CASE(64, 6);   // 208/16: 170 tokens
  ATTN_CASE(64, 8);   // 240/16: 226 tokens
  ATTN_CASE(64, 9);   // 224/14 with d_h = 64: 257 tokens (ViT-L/14)
#undef ATTN_CASE
  return fail(SSP2_EINVAL, "attention kernel not instantiated for d_h=%d, tokens=%d", e->dh, e->tokens);
}

static int act_l2_impl(void* stream, const void* act, int dtype, int n, RowMap rm, int d, int ld, int chain, int group,
                       float* norms_ws, float* out, size_t out_stride);
// The fused score finish: the fc1 epilogue's slab -> per-sample norms -> per-group sums.  The two launches the forward's hook issues
// (score_finish) and the ones ssp2_score_finish issues: one function, so that the entry is the forward's launch and not a copy of it.
static int score_finish_fused(hipStream_t s, const float* slab, int n, RowMap rm, int grp, int ld, int chain, float* norms, float* out,
                              size_t out_stride) {
  const int n_groups = (n + grp - 1) / grp;
  hipLaunchKernelGGL(score_norms_from_slab_kernel, dim3((ld + 255) / 256, n), dim3(256), 0, s, slab, norms, n, rm, ld, chain);
  hipLaunchKernelGGL(score_colsum_kernel, dim3((ld + 255) / 256, n_groups), dim3(256), 0, s, norms, out, out_stride, n, grp, ld, chain);
  HIPCHK(hipGetLastError());
  return 0;
}
// the unfused scoring path (models with < 128 tokens) reads the bf16 activation back: it stays on the bf16 kernels
static inline bool fused_ok_for_fp8(int score_site, int tokens) { return score_site == 0 || tokens >= GEMM_BM; }

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" {

int ssp2_abi_version(void) { return SSP2_ABI_VERSION; }
const char* ssp2_last_error(void) { return g_err.c_str(); }

int ssp2_create(const ssp2_vit_desc* desc, ssp2_handle* out) { return ssp2_create_ext(desc, nullptr, nullptr, out); }

int ssp2_create_opts(const ssp2_vit_desc* desc, const int32_t* opt, ssp2_handle* out) { return ssp2_create_ext(desc, opt, nullptr, out); }

int ssp2_create_ext(const ssp2_vit_desc* desc, const int32_t* opt, const ssp2_vit_ext* ext, ssp2_handle* out) {
  const ssp2_token_layout lay{ext ? ext->prefix_tokens : 1, ext ? ext->dist_head : 0, 0, 1};
  return ssp2_create_layout(desc, opt, &lay, out);
}

int ssp2_create_layout(const ssp2_vit_desc* desc, const int32_t* opt, const ssp2_token_layout* layout, ssp2_handle* out) {
  if (!desc || !out || !desc->d_int) return fail(SSP2_EINVAL, "null argument");
  const int prefix = layout ? layout->prefix_tokens : 1, dist_head = layout ? layout->dist_head : 0;
  const int reg_tokens = layout ? layout->reg_tokens : 0, pos_prefix_rows = layout ? layout->pos_prefix_rows : 1;
  if (reg_tokens < 0 || reg_tokens > 8) return fail(SSP2_EINVAL, "reg_tokens %d: 0 to 8 register tokens", reg_tokens);
  if (pos_prefix_rows < 0 || pos_prefix_rows > 1)
    return fail(SSP2_EINVAL, "pos_prefix_rows %d: 1 (positions for every token) or 0 (class-free positions: the patches' rows only)", pos_prefix_rows);
  if (reg_tokens > 0 && prefix != 1 + reg_tokens)
    return fail(SSP2_EINVAL, "prefix_tokens %d: CLS + reg_tokens = %d register tokens are %d prefix tokens", prefix, reg_tokens, 1 + reg_tokens);
  if (prefix < 1 || (reg_tokens == 0 && prefix > 2)) return fail(SSP2_EINVAL, "prefix_tokens %d: 1 (CLS) or 2 (CLS + distillation token)", prefix);
  if (dist_head < 0 || dist_head > 1) return fail(SSP2_EINVAL, "dist_head %d: 0 (CLS head) or 1 (CLS and distillation heads averaged)", dist_head);
  if (dist_head && reg_tokens > 0) return fail(SSP2_EINVAL, "dist_head = 1 with reg_tokens = %d: a distilled model has no register tokens", reg_tokens);
  if (dist_head && prefix != 2) return fail(SSP2_EINVAL, "dist_head = 1 reads the distillation token: it needs prefix_tokens = 2 (got %d)", prefix);
  if (!pos_prefix_rows && (dist_head || (reg_tokens == 0 && prefix == 2)))
    return fail(SSP2_EINVAL, "pos_prefix_rows = 0 with a distillation token (prefix_tokens %d, dist_head %d): a distilled model has positions for every token", prefix, dist_head);
  if (opt) {
    for (int i = 0; i < SSP2_OPT_COUNT; ++i)
      if (opt[i] < -1) return fail(SSP2_EINVAL, "option %d: override %d (-1 = environment default)", i, opt[i]);
    if (opt[SSP2_OPT_ATTN_STREAM] > 2) return fail(SSP2_EINVAL, "SSP2_OPT_ATTN_STREAM takes 0, 1 or 2");
  }
  const ssp2_vit_desc& d = *desc;
  if (d.img <= 0 || d.patch <= 0 || d.img % d.patch) return fail(SSP2_EINVAL, "img %d not divisible by patch %d", d.img, d.patch);
  if (d.dim <= 0 || d.dim % 64 || d.dim > 2048) return fail(SSP2_EINVAL, "dim %d must be a multiple of 64, <= 2048", d.dim);
  if (d.heads <= 0 || d.dim % d.heads) return fail(SSP2_EINVAL, "dim %d not divisible by heads %d", d.dim, d.heads);
  if (d.depth <= 0 || d.classes <= 0 || d.max_images <= 0) return fail(SSP2_EINVAL, "depth/classes/max_images must be positive");
  auto* e = new ssp2_engine();      // (host state only until the geometry has been accepted: every SSP2_EINVAL below comes before the device is touched)
  e->d = d;
  {   // option defaults, each overridable ONCE by its environment variable (read here, never on a launch path)
    auto env_int = [](const char* name, int dflt) { const char* v = getenv(name); return (v && *v) ? atoi(v) : dflt; };
    e->opt[SSP2_OPT_ZIGZAG] = env_int("SSP2_ZIGZAG", 1);
    e->opt[SSP2_OPT_ATTN_PERSIST] = env_int("SSP2_ATTN_PERSIST", 1);
#ifdef SSP2_LAB
    e->opt[SSP2_OPT_LN_FUSION] = env_int("SSP2_LN_FUSION", 0);
#else
    e->opt[SSP2_OPT_LN_FUSION] = 0;
#endif
    e->opt[SSP2_OPT_BIG_TILES] = getenv("SSP2_NO_BIG_TILES") ? 0 : 1;
    e->opt[SSP2_OPT_FC1_BIG_TILES] = getenv("SSP2_FC1_SMALL_TILES") ? 0 : 1;
#ifdef SSP2_LAB
    e->opt[SSP2_OPT_GROUP256] = env_int("SSP2_GROUP256", 0);
#else
    e->opt[SSP2_OPT_GROUP256] = 0;
#endif
    e->opt[SSP2_OPT_PATCH_LDS] = env_int("SSP2_PATCH_LDS", 1);
    e->opt[SSP2_OPT_ATTN_STAGGER] = env_int("SSP2_ATTN_STAGGER", 0);
    e->opt[SSP2_OPT_FP8_PROJ] = env_int("SSP2_FP8_PROJ", 1);
    e->opt[SSP2_OPT_BIG_TILE_MIN_ROWS] = std::max(256, env_int("SSP2_BIG_TILE_MIN_ROWS", kBigTileMinRowsDefault));
    e->opt[SSP2_OPT_NT_STORES] = env_int("SSP2_NT_STORES", 1);
    e->opt[SSP2_OPT_ATTN_LIVE] = env_int("SSP2_ATTN_LIVE", 1);
#ifdef SSP2_LAB
    e->opt[SSP2_OPT_DEFER_RESID] = env_int("SSP2_DEFER_RESID", 0);
#else
    e->opt[SSP2_OPT_DEFER_RESID] = 0;
#endif
    e->opt[SSP2_OPT_ATTN_STREAM] = std::max(0, std::min(2, env_int("SSP2_ATTN_STREAM", 0)));
    e->opt[SSP2_OPT_STREAM_FP8] = env_int("SSP2_STREAM_FP8", 0) ? 1 : 0;
  }
  if (opt) {   // explicit overrides go through the same checks as ssp2_set_option (the geometry is not known yet: checked below)
    for (int i = 0; i < SSP2_OPT_COUNT; ++i) {
      if (opt[i] < 0) continue;
      const int v = opt[i];
      bool bad = (i == SSP2_OPT_LN_FUSION && v > 2) || (i == SSP2_OPT_BIG_TILE_MIN_ROWS && v < 256);
#ifndef SSP2_LAB
      bad = bad || ((i == SSP2_OPT_LN_FUSION || i == SSP2_OPT_DEFER_RESID || i == SSP2_OPT_GROUP256) && v != 0);
#endif
      if (bad) { delete e; return fail(SSP2_EINVAL, "option %d: override %d not accepted", i, v); }
      e->opt[i] = v;
    }
  }
  e->d_int.assign(d.d_int, d.d_int + d.depth);
  e->d.d_int = e->d_int.data();
  e->side = d.img / d.patch;
  e->patches = e->side * e->side;
  e->prefix = prefix; e->dist_head = dist_head; e->tail_rows = dist_head ? 2 : 1;
  e->reg_tokens = reg_tokens; e->pos_prefix_rows = pos_prefix_rows;
  e->tokens = e->patches + prefix;
  e->dh = d.dim / d.heads;
  e->kpe = 3 * d.patch * d.patch;
  e->kpe_pad = ceil_to(e->kpe, GEMM_BK);
  if (!(e->dh == 16 || e->dh == 64 || e->dh == 80)) {
    delete e;
    return fail(SSP2_EINVAL, "head dim %d unsupported (16, 64, 80)", d.dim / d.heads);
  }
  if (!attn_supported(e->dh, e->tokens, e->opt[SSP2_OPT_ATTN_STREAM])) {
    const int dh = e->dh, tk = e->tokens;
    delete e;
    if (attn_stream_ok(dh, tk))
      return fail(SSP2_EINVAL, "no resident attention kernel for head dim %d with %d tokens (head dim 64: up to 288 tokens); the key-streaming "
                               "kernel takes it when opted in: SSP2_OPT_ATTN_STREAM = 1 (environment SSP2_ATTN_STREAM=1, VitEngine(attn_stream=1), "
                               "CLI --long-sequences)", dh, tk);
    return fail(SSP2_EINVAL, "no attention kernel for head dim %d with %d tokens (head dim 64: up to 288 tokens, up to %d with SSP2_OPT_ATTN_STREAM; "
                             "80: 257..288; 16: up to 32)", dh, tk, ATTN_STREAM_MAX_TOKENS);
  }
  int dev_count = 0;
  if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) {
    delete e;
    return fail(SSP2_EHIP, "no HIP device visible: libssp2vit has no CPU path");
  }
  {
    int dev = 0; hipDeviceProp_t pr;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) e->n_cu = pr.multiProcessorCount;
    e->dev = (dev >= 0 && dev < kMaxDevices) ? dev : 0;
  }
  int rc = 0;
#define TRY(x) do { if ((rc = (x))) { ssp2_destroy(e); return rc; } } while (0)
#define TRYA(x) do { if (int rc_ = (x)) return rc_; } while (0)
  auto alloc_all = [&]() -> int {
  TRYA(mat_alloc(e, e->patch, d.dim, e->kpe));
  TRYA(mat_alloc(e, e->head, d.classes, d.dim));
  if (e->dist_head) TRYA(mat_alloc(e, e->head_dist, d.classes, d.dim));
  TRYA(dalloc(e, &e->cls, d.dim, false));
  if (e->prefix == 2 && !e->reg_tokens) TRYA(dalloc(e, &e->dist, d.dim, false));
  if (e->reg_tokens) TRYA(dalloc(e, &e->reg, (size_t)e->reg_tokens * d.dim, false));
  TRYA(dalloc(e, &e->pos, e->pos_rows() * d.dim, false));
  TRYA(dalloc(e, &e->lnf_g, d.dim, false));
  TRYA(dalloc(e, &e->lnf_b, d.dim, false));
  e->layers.resize(d.depth);
  e->ld_int_max = 0;
  for (int l = 0; l < d.depth; ++l) {
    Layer& L = e->layers[l];
    L.d_int = e->d_int[l];
    if (L.d_int <= 0) return fail(SSP2_EINVAL, "d_int[%d] = %d", l, L.d_int);
    L.ld_int = ceil_to(L.d_int, GEMM_BK);
    e->ld_int_max = L.ld_int > e->ld_int_max ? L.ld_int : e->ld_int_max;
    TRYA(dalloc(e, &L.ln1_g, d.dim, false)); TRYA(dalloc(e, &L.ln1_b, d.dim, false));
    TRYA(dalloc(e, &L.ln2_g, d.dim, false)); TRYA(dalloc(e, &L.ln2_b, d.dim, false));
    TRYA(dalloc(e, &L.ls[0], (size_t)ceil_to(d.dim, 256), false)); TRYA(dalloc(e, &L.ls[1], (size_t)ceil_to(d.dim, 256), false));      // (padded like a bias, pad zero)
    TRYA(mat_alloc(e, L.qkv, 3 * d.dim, d.dim));
    TRYA(mat_alloc(e, L.proj, d.dim, d.dim));
    TRYA(mat_alloc(e, L.fc1, L.d_int, d.dim));
    TRYA(mat_alloc(e, L.fc2, d.dim, L.d_int));
  }
  e->rows_cap = (long)d.max_images * e->tokens + 16 * 256;     // slack: up to 16 padded slabs per call
  const size_t M = (size_t)e->rows_cap;
  const size_t tiles_m = (M + GEMM_BM - 1) / GEMM_BM;
  // (a_pe, the im2col image of the old patch-embed path, is allocated only if SSP2_OPT_PATCH_LDS is switched off: see ssp2_embed)
  TRYA(dalloc(e, &e->hbuf, M * d.dim, true));
  TRYA(dalloc(e, &e->qkvbuf, M * 3 * d.dim, true, false));      // every row of a launch is written by the QKV GEMM before the attention reads it
  TRYA(dalloc(e, &e->obuf, M * d.dim, true));
  TRYA(dalloc(e, &e->actbuf, M * e->ld_int_max, true, false));   // ... and by fc1 before fc2 reads it (pad columns included: zero weight rows)
  if (e->tokens < GEMM_BM) TRYA(dalloc(e, &e->prebuf, M * e->ld_int_max, true, false));
  TRYA(dalloc(e, &e->slab, tiles_m * 2 * e->ld_int_max, true));
  TRYA(dalloc(e, &e->norms, (size_t)2 * d.max_images * e->ld_int_max, true));   // [2 token halves][n][ld] for the standalone L2 kernel
  const size_t pre_rows = (size_t)std::min(e->prefix, 2) * d.max_images;   // the tail's and the head's rows: tail_rows (<= 2) per image; register tokens add none
  TRYA(dalloc(e, &e->cls_h, pre_rows * d.dim, true));
  TRYA(dalloc(e, &e->x_cls, pre_rows * d.dim, true));
  TRYA(dalloc(e, &e->q_cls, pre_rows * d.dim, true));
  TRYA(dalloc(e, &e->o_cls, pre_rows * d.dim, true));
  TRYA(dalloc(e, &e->h_cls, pre_rows * d.dim, true));
  TRYA(dalloc(e, &e->act_cls, pre_rows * e->ld_int_max, true));
  // logits scratch: [n, classes]; with the distillation head the two heads' outputs and their mean
  TRYA(dalloc(e, &e->logits, (size_t)(e->dist_head ? 3 : 1) * d.max_images * d.classes, true));
  TRYA(dalloc(e, &e->ln_sync, (size_t)16 + (M + 255) / 256 + 1, true));
#ifdef SSP2_LAB
  TRYA(dalloc(e, &e->dg_scratch, (size_t)std::max(e->n_cu, 1) * 32768, true));      // 128 KiB per workgroup of the persistent GEMM (deferred residual, lab build)
#endif
    return 0;
  };
  e->arena_mode = 1;                                            // sizes
  TRY(alloc_all());
  for (int k = 0; k < 2; ++k) {
    void* q = nullptr;
    if (hipMalloc(&q, std::max<size_t>(e->arena_need[k], 256)) != hipSuccess) { ssp2_destroy(e); return fail(SSP2_ENOMEM, "hipMalloc(%zu) failed", e->arena_need[k]); }
    e->allocs.push_back(q);
    e->arena_cur[k] = (char*)q;
  }
  if (hipMemset(e->arena_cur[0], 0, std::max<size_t>(e->arena_need[0], 256)) != hipSuccess) { ssp2_destroy(e); return fail(SSP2_EHIP, "hipMemset failed"); }
  e->arena_mode = 2;                                            // pointers
  e->ws_bytes = e->weight_bytes = 0;
  TRY(alloc_all());
  e->arena_mode = 0;
#undef TRYA
#undef TRY
#ifdef SSP2_LAB
  {   // the fused LayerNorm (lab build) trusts the hardware's XCC_ID to name the L2 a workgroup sits behind: look at what it reports once
    unsigned int* ids = nullptr;
    const int nb = e->n_cu > 0 ? 4 * e->n_cu : 1024;
    if (hipMalloc((void**)&ids, nb * sizeof(unsigned int)) == hipSuccess) {
      std::vector<unsigned int> h(nb, 0xffffffffu);
      hipLaunchKernelGGL(xcc_probe_kernel, dim3(nb), dim3(64), 0, e->stream, ids);
      if (hipStreamSynchronize(e->stream) == hipSuccess && hipMemcpy(h.data(), ids, nb * sizeof(unsigned int), hipMemcpyDeviceToHost) == hipSuccess) {
        unsigned seen = 0; bool bad = false;
        for (unsigned v : h) { if (v > 7) bad = true; else seen |= 1u << v; }
        e->xcc_ok = !bad && seen != 0;
        e->n_xcc_seen = __builtin_popcount(seen);
      }
      hipFree(ids);
    }
  }
#endif
  *out = e;
  return 0;
}

int ssp2_destroy(ssp2_handle e) {
  if (!e) return 0;
  hipStreamSynchronize(e->stream);
  for (auto& pr : e->prof_events) { hipEventDestroy(pr.a); hipEventDestroy(pr.b); }
  for (void* p : e->allocs) hipFree(p);
  hipFree(e->prune_t1); hipFree(e->prune_t2); hipFree(e->prune_tb); hipFree(e->prune_keep);
  if (e->stage_f32) hipFree(e->stage_f32);
  for (auto ev : e->keep_ev) if (ev) hipEventDestroy(ev);
  if (e->keep_pin) hipHostFree(e->keep_pin);
  delete e;
  return 0;
}

int ssp2_set_stream(ssp2_handle e, void* s) {
  if (!e) return fail(SSP2_EINVAL, "null handle");
  e->stream = (hipStream_t)s;
  return 0;
}

int ssp2_fp8_calibrate_begin(ssp2_handle e) {
  if (!e) return fail(SSP2_EINVAL, "null handle");
  if (!e->fp8 || !e->attn_amax) return fail(SSP2_ESTATE, "fp8 calibration needs ssp2_set_precision(h, SSP2_PREC_FP8) first");
  HIPCHK(hipMemsetAsync(e->attn_amax, 0, (size_t)e->d.depth * 4, e->stream));
  if (e->act8_top) HIPCHK(hipMemsetAsync(e->act8_top, 0, 8, e->stream));
  e->fp8_calibrating = true;
  return 0;
}
int ssp2_fp8_calibrate_end(ssp2_handle e, float headroom) {
  if (!e) return fail(SSP2_EINVAL, "null handle");
  if (!e->fp8_calibrating) return fail(SSP2_ESTATE, "ssp2_fp8_calibrate_end without ssp2_fp8_calibrate_begin");
  e->fp8_calibrating = false;
  if (!(headroom >= 1.0f)) headroom = 1.0f;
  std::vector<float> amax(e->d.depth, 0.f);
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(amax.data(), e->attn_amax, (size_t)e->d.depth * 4, hipMemcpyDeviceToHost));
  for (int l = 0; l < e->d.depth; ++l) {
    if (!(amax[l] > 0.f) || !std::isfinite(amax[l])) continue;                 // block not seen (skipped / dropped attention): keeps its scale
    int ex = (int)floorf(log2f(448.0f / (amax[l] * headroom)));
    ex = std::max(-8, std::min(10, ex));
    e->layers[l].o8_scale = ldexpf(1.0f, ex);
  }
  return 0;
}
float ssp2_fp8_attn_scale(ssp2_handle e, int layer) {
  if (!e || layer < 0 || layer >= e->d.depth) return 0.f;
  return e->layers[layer].o8_scale;
}
int ssp2_fp8_set_attn_scale(ssp2_handle e, int layer, float scale) {
  if (!e || layer < 0 || layer >= e->d.depth) return fail(SSP2_EINVAL, "bad layer");
  int ex = 0;
  if (!(scale > 0.f) || frexpf(scale, &ex) != 0.5f) return fail(SSP2_EINVAL, "the scale must be a power of two > 0 (got %g)", scale);
  e->layers[layer].o8_scale = scale;
  return 0;
}

int ssp2_set_cu_limit(ssp2_handle e, int n_cu) {
  if (!e) return fail(SSP2_EINVAL, "null handle");
  int dev = 0; hipDeviceProp_t pr;
  int phys = 256;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) phys = pr.multiProcessorCount;
  e->n_cu = (n_cu <= 0 || n_cu > phys) ? phys : n_cu;
  return 0;
}
int ssp2_set_option(ssp2_handle e, int option, int value) {
  if (!e) return fail(SSP2_EINVAL, "null handle");
  if (option < 0 || option >= SSP2_OPT_END) return fail(SSP2_EINVAL, "unknown option %d", option);
  if (option == SSP2_OPT_LN_FUSION && (value < 0 || value > 2)) return fail(SSP2_EINVAL, "SSP2_OPT_LN_FUSION takes 0, 1 or 2");
  if (option == SSP2_OPT_GROUP256 && value < 0) return fail(SSP2_EINVAL, "SSP2_OPT_GROUP256 takes 100 * GM + GN >= 0");
  if (option == SSP2_OPT_BIG_TILE_MIN_ROWS && value < 256) return fail(SSP2_EINVAL, "SSP2_OPT_BIG_TILE_MIN_ROWS takes >= 256 rows");
#ifndef SSP2_LAB
  if ((option == SSP2_OPT_LN_FUSION || option == SSP2_OPT_DEFER_RESID || option == SSP2_OPT_GROUP256) && value != 0)
    return fail(SSP2_ESTATE, "option %d (LayerNorm fusion / deferred residual / column-group tile order) exists in the lab build only: "
                             "lib/libssp2vit_lab.so (scripts/build_variant.py lab -DSSP2_LAB=1; VitEngine(lib_variant=\"lab\"))", option);
#endif
  if (option == SSP2_OPT_ATTN_STREAM) {
    if (value < 0 || value > 2) return fail(SSP2_EINVAL, "SSP2_OPT_ATTN_STREAM takes 0, 1 or 2");
    if (!attn_supported(e->dh, e->tokens, value))
      return fail(SSP2_ESTATE, "SSP2_OPT_ATTN_STREAM = %d: head dim %d with %d tokens has no resident attention kernel", value, e->dh, e->tokens);
    if (e->fp8 && attn_streams(value, e->dh, e->tokens) && !e->opt[SSP2_OPT_STREAM_FP8]) return fail(SSP2_ESTATE, "SSP2_OPT_ATTN_STREAM = %d: the key-streaming attention is bf16 only (engine is in fp8)", value);
  }
  if (option == SSP2_OPT_STREAM_FP8) {
    if (value < 0 || value > 1) return fail(SSP2_EINVAL, "SSP2_OPT_STREAM_FP8 takes 0 or 1");
    if (!value && e->fp8 && attn_streaming(e))
      return fail(SSP2_ESTATE, "SSP2_OPT_STREAM_FP8 = 0: this engine is in fp8 on the key-streaming attention (SSP2_OPT_FP8_PROJ = 0 keeps its attention output on bf16)");
  }
  e->opt[option] = value;
  return 0;
}
int ssp2_get_option(ssp2_handle e, int option) {
  if (!e || option < 0 || option >= SSP2_OPT_END) return fail(SSP2_EINVAL, "bad option query");
  return e->opt[option];
}
int ssp2_tokens(ssp2_handle e) { return e ? e->tokens : SSP2_EINVAL; }
int ssp2_query(ssp2_handle e, int what) {
  if (!e) return SSP2_EINVAL;
  switch (what) {
    case SSP2_Q_DIM: return e->d.dim;
    case SSP2_Q_DEPTH: return e->d.depth;
    case SSP2_Q_CLASSES: return e->d.classes;
    case SSP2_Q_SCORE_LD: { int m = 0; for (auto& L : e->layers) m = std::max(m, L.ld_int); return m; }
    case SSP2_Q_MAX_IMAGES: return e->d.max_images;
    case SSP2_Q_TOKENS: return e->tokens;
    case SSP2_Q_IMG: return e->d.img;
    case SSP2_Q_FP8_FC2_TOP_CODES: {
      if (!e->act8_top) return 0;
      unsigned long long v = 0;
      if (hipStreamSynchronize(e->stream) != hipSuccess || hipMemcpy(&v, e->act8_top, 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(SSP2_EHIP, "reading the top-code counter failed");
      return (int)std::min<unsigned long long>(v, 0x7fffffffull);
    }
    case SSP2_Q_LAB_BUILD:
#ifdef SSP2_LAB
      return 1;
#else
      return 0;
#endif
    case SSP2_Q_FP8_SATURATED:
    case SSP2_Q_FP8_SATURATED_RESET: {
      if (!e->fp8_sat) return 0;
      unsigned int v = 0;
      if (hipStreamSynchronize(e->stream) != hipSuccess || hipMemcpy(&v, e->fp8_sat, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(SSP2_EHIP, "reading the fp8 saturation counter failed");
      if (what == SSP2_Q_FP8_SATURATED_RESET && hipMemset(e->fp8_sat, 0, sizeof(v)) != hipSuccess) return fail(SSP2_EHIP, "resetting the fp8 saturation counter failed");
      return (int)std::min<unsigned int>(v, 0x7fffffffu);
    }
    default: return fail(SSP2_EINVAL, "unknown query %d", what);
  }
}
long ssp2_rows(ssp2_handle e, int n, int group) { return e ? total_rows(make_rowmap(e->tokens, n, group), n) : SSP2_EINVAL; }
size_t ssp2_workspace_bytes(ssp2_handle e) { return e ? e->ws_bytes : 0; }

// Weight ingest.  The fp32 source (nn.Linear [out,in] as stored) is rounded to bf16 and laid out with the padded
// leading dimension ON THE DEVICE (convert_pad_bf16_kernel): a host source costs one hipMemcpy of the fp32 bytes into a
// staging buffer, a device source (a module that already lives on the GPU) costs nothing but the kernel.  Round 1
// converted on the host in a single-threaded double loop over every weight — seconds for ViT-B/16 inside the caller's
// prune bracket whenever the host API had to (re)build its engine.
static int stage_fp32(ssp2_engine* e, const float* src, size_t numel, bool src_on_device, const float** out) {
  if (src_on_device) { *out = src; return 0; }
  if (e->stage_cap < numel) {
    if (e->stage_f32) hipFree(e->stage_f32);
    e->stage_f32 = nullptr; e->stage_cap = 0;
    if (hipMalloc((void**)&e->stage_f32, numel * 4) != hipSuccess) return fail(SSP2_ENOMEM, "hipMalloc(%zu) for the weight staging buffer failed", numel * 4);
    e->stage_cap = numel;
  }
  HIPCHK(hipMemcpyAsync(e->stage_f32, src, numel * 4, hipMemcpyHostToDevice, e->stream));
  *out = e->stage_f32;
  return 0;
}
static int upload_matrix(ssp2_engine* e, Mat& m, const float* src, size_t numel, bool dev) {
  if (numel != (size_t)m.rows * m.cols) return fail(SSP2_EINVAL, "matrix expects %d x %d = %zu values, got %zu", m.rows, m.cols, (size_t)m.rows * m.cols, numel);
  const float* d = nullptr;
  int rc;
  if ((rc = stage_fp32(e, src, numel, dev, &d))) return rc;
  const long total = (long)m.rows_pad * (m.ld / 8);
  hipLaunchKernelGGL(convert_pad_bf16_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, e->stream, d, m.w, m.rows, m.cols, m.rows_pad, m.ld);
  HIPCHK(hipGetLastError());
  if (!dev) HIPCHK(hipStreamSynchronize(e->stream));     // the staging buffer is reused by the next tensor; the host source may go away
  m.w_set = true;
  return 0;
}
static int upload_bias(ssp2_engine* e, Mat& m, const float* src, size_t numel, bool dev) {
  if (numel != (size_t)m.rows) return fail(SSP2_EINVAL, "bias expects %d values, got %zu", m.rows, numel);
  const float* d = nullptr;
  int rc;
  if ((rc = stage_fp32(e, src, numel, dev, &d))) return rc;
  hipLaunchKernelGGL(round_bias_kernel, dim3((m.rows_pad + 255) / 256), dim3(256), 0, e->stream, d, m.b, m.rows, m.rows_pad);   // autocast casts the bias to bf16 too
  HIPCHK(hipGetLastError());
  if (!dev) HIPCHK(hipStreamSynchronize(e->stream));
  m.b_set = true;
  return 0;
}
static int upload_f32(ssp2_engine* e, float* dst, const float* src, size_t numel, size_t expect, bool* flag, bool dev) {
  if (numel != expect) return fail(SSP2_EINVAL, "vector expects %zu values, got %zu", expect, numel);
  HIPCHK(hipMemcpyAsync(dst, src, numel * 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
  if (!dev) HIPCHK(hipStreamSynchronize(e->stream));
  *flag = true;
  return 0;
}

// where a tensor kind goes: a weight matrix's bf16 image, its bias, or an fp32 vector kept as it is
struct IngestTarget { int type = 2; Mat* m = nullptr; float* dst = nullptr; size_t expect = 0; bool* flag = nullptr; };
static int resolve_tensor(ssp2_engine* e, int kind, int layer, IngestTarget* t) {
  const int D = e->d.dim;
  const bool per_layer = kind >= SSP2_T_LN1_G && kind <= SSP2_T_FC2_B;
  if (per_layer && (layer < 0 || layer >= e->d.depth)) return fail(SSP2_EINVAL, "layer %d out of range", layer);
  Layer* L = per_layer ? &e->layers[layer] : nullptr;
  auto mat = [&](Mat& m) { t->type = 0; t->m = &m; t->expect = (size_t)m.rows * m.cols; return 0; };
  auto bias = [&](Mat& m) { t->type = 1; t->m = &m; t->expect = (size_t)m.rows; return 0; };
  auto vec = [&](float* dst, size_t expect, bool* flag) { t->type = 2; t->dst = dst; t->expect = expect; t->flag = flag; return 0; };
  switch (kind) {
    case SSP2_T_PATCH_W: return mat(e->patch);
    case SSP2_T_PATCH_B: return bias(e->patch);
    case SSP2_T_CLS: return vec(e->cls, D, &e->misc_set[0]);
    case SSP2_T_POS: return vec(e->pos, e->pos_rows() * D, &e->misc_set[1]);      // (class-free positions: the patches' rows only)
    case SSP2_T_LN1_G: return vec(L->ln1_g, D, &L->ln_set[0]);
    case SSP2_T_LN1_B: return vec(L->ln1_b, D, &L->ln_set[1]);
    case SSP2_T_LN2_G: return vec(L->ln2_g, D, &L->ln_set[2]);
    case SSP2_T_LN2_B: return vec(L->ln2_b, D, &L->ln_set[3]);
    case SSP2_T_QKV_W: return mat(L->qkv);
    case SSP2_T_QKV_B: return bias(L->qkv);
    case SSP2_T_PROJ_W: return mat(L->proj);
    case SSP2_T_PROJ_B: return bias(L->proj);
    case SSP2_T_FC1_W: return mat(L->fc1);
    case SSP2_T_FC1_B: return bias(L->fc1);
    case SSP2_T_FC2_W: return mat(L->fc2);
    case SSP2_T_FC2_B: return bias(L->fc2);
    case SSP2_T_LNF_G: return vec(e->lnf_g, D, &e->misc_set[2]);
    case SSP2_T_LNF_B: return vec(e->lnf_b, D, &e->misc_set[3]);
    case SSP2_T_HEAD_W: return mat(e->head);
    case SSP2_T_HEAD_B: return bias(e->head);
    case SSP2_T_DIST:
      if (!e->dist) return fail(SSP2_EINVAL, "tensor kind %d (distillation token): this engine has one prefix token (ssp2_create_ext prefix_tokens = 2)", kind);
      return vec(e->dist, D, &e->dist_set);
    case SSP2_T_HEAD_DIST_W:
    case SSP2_T_HEAD_DIST_B:
      if (!e->dist_head) return fail(SSP2_EINVAL, "tensor kind %d (distillation head): this engine has no distillation head (ssp2_create_ext dist_head = 1)", kind);
      return kind == SSP2_T_HEAD_DIST_W ? mat(e->head_dist) : bias(e->head_dist);
    default: return fail(SSP2_EINVAL, "unknown tensor kind %d", kind);
  }
}

static int load_tensor_impl(ssp2_handle e, int kind, int layer, const float* src, size_t numel, bool dev) {
  if (!e || !src) return fail(SSP2_EINVAL, "null argument");
  IngestTarget t;
  if (int rc = resolve_tensor(e, kind, layer, &t)) return rc;
  if (t.type == 0) return upload_matrix(e, *t.m, src, numel, dev);
  if (t.type == 1) return upload_bias(e, *t.m, src, numel, dev);
  return upload_f32(e, t.dst, src, numel, t.expect, t.flag, dev);
}
int ssp2_load_tensor(ssp2_handle e, int kind, int layer, const float* host, size_t numel) { return load_tensor_impl(e, kind, layer, host, numel, false); }
int ssp2_load_tensor_dev(ssp2_handle e, int kind, int layer, const float* dev_ptr, size_t numel) { return load_tensor_impl(e, kind, layer, dev_ptr, numel, true); }

// Many device-resident tensors at once (a live module's ~150 parameters): every entry is validated first — nothing is enqueued when one
// is wrong —, then the batch goes out in launches of up to kIngestBatch tensors (ingest_batch_kernel; the descriptors are the kernel
// argument).  Same bits as ssp2_load_tensor_dev entry by entry.
int ssp2_load_tensors_dev(ssp2_handle e, int count, const int* kinds, const int* layers, const float* const* dev_ptrs, const size_t* numels) {
  if (!e || count < 0 || (count && (!kinds || !layers || !dev_ptrs || !numels))) return fail(SSP2_EINVAL, "null argument");
  std::vector<IngestTarget> ts((size_t)count);
  for (int i = 0; i < count; ++i) {
    if (!dev_ptrs[i]) return fail(SSP2_EINVAL, "entry %d: null tensor", i);
    if (int rc = resolve_tensor(e, kinds[i], layers[i], &ts[i])) return rc;
    if (numels[i] != ts[i].expect) return fail(SSP2_EINVAL, "entry %d (kind %d, layer %d) expects %zu values, got %zu", i, kinds[i], layers[i], ts[i].expect, numels[i]);
  }
  for (int at = 0; at < count; at += kIngestBatch) {
    IngestBatch b;
    b.count = std::min(kIngestBatch, count - at);
    unsigned long work = 0;
    for (int k = 0; k < b.count; ++k) {
      const IngestTarget& t = ts[at + k];
      IngestDesc& d = b.d[k];
      d.src = dev_ptrs[at + k]; d.type = t.type;
      if (t.type == 0) { d.dst = t.m->w; d.rows = t.m->rows; d.cols = t.m->cols; d.rows_pad = t.m->rows_pad; d.ld = t.m->ld; work += (unsigned long)t.m->rows_pad * (t.m->ld / 8); }
      else if (t.type == 1) { d.dst = t.m->b; d.rows = t.m->rows; d.cols = 1; d.rows_pad = t.m->rows_pad; d.ld = 0; work += (unsigned long)(t.m->rows_pad + 7) / 8; }
      else { d.dst = t.dst; d.rows = (int)t.expect; d.cols = 1; d.rows_pad = (int)t.expect; d.ld = 0; work += (unsigned long)(t.expect + 7) / 8; }
      if (work > 0xffffffffUL) return fail(SSP2_EINVAL, "ingest batch too large");
      d.work_end = (unsigned)work;
    }
    if (!work) continue;
    hipLaunchKernelGGL(ingest_batch_kernel, dim3((unsigned)std::min<unsigned long>((work + 255) / 256, 8192)), dim3(256), 0, e->stream, b);
    HIPCHK(hipGetLastError());
  }
  for (int i = 0; i < count; ++i) {
    if (ts[i].type == 0) ts[i].m->w_set = true; else if (ts[i].type == 1) ts[i].m->b_set = true; else *ts[i].flag = true;
  }
  return 0;
}

// LayerScale of one residual branch: fp32 in, fp32 held (the parameter is never rounded: autocast multiplies by it in fp32)
static int set_layer_scale_impl(ssp2_engine* e, Layer& L, int branch, const float* gamma, bool dev) {
  const int D = e->d.dim;
  HIPCHK(hipMemcpyAsync(L.ls[branch], gamma, (size_t)D * 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
  if (!dev) HIPCHK(hipStreamSynchronize(e->stream));
  L.ls_set[branch] = true;
  return 0;
}
int ssp2_set_layer_scale(ssp2_handle e, int layer, int branch, const float* gamma, int on_device) {
  if (!e) return fail(SSP2_EINVAL, "null handle");
  if (layer < 0 || layer >= e->d.depth) return fail(SSP2_EINVAL, "set_layer_scale: layer %d out of range [0, %d)", layer, e->d.depth);
  if (branch < 0 || branch > 1) return fail(SSP2_EINVAL, "set_layer_scale: branch %d (0 = attention, 1 = MLP)", branch);
  if (!gamma) return fail(SSP2_EINVAL, "set_layer_scale: null gamma");
  return set_layer_scale_impl(e, e->layers[layer], branch, gamma, on_device != 0);
}

// Register tokens: fp32 in, fp32 held (parameters: the concat with the fp32 position sum keeps them as they are)
static int set_reg_tokens_impl(ssp2_engine* e, const float* reg, bool dev) {
  HIPCHK(hipMemcpyAsync(e->reg, reg, (size_t)e->reg_tokens * e->d.dim * 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
  if (!dev) HIPCHK(hipStreamSynchronize(e->stream));
  e->reg_set = true;
  return 0;
}
int ssp2_set_reg_tokens(ssp2_handle e, const float* reg, int count, int on_device) {
  if (!e) return fail(SSP2_EINVAL, "null handle");
  if (count != e->reg_tokens || count <= 0)
    return fail(SSP2_EINVAL, "set_reg_tokens: count %d, this engine has reg_tokens = %d (ssp2_create_layout)", count, e->reg_tokens);
  if (!reg) return fail(SSP2_EINVAL, "set_reg_tokens: null reg");
  return set_reg_tokens_impl(e, reg, on_device != 0);
}

static int check_n(ssp2_engine* e, int n, int group = 0) {
  if (!e) return fail(SSP2_EINVAL, "null handle");
  if (n <= 0 || n > e->d.max_images) return fail(SSP2_ESTATE, "n=%d outside (0, max_images=%d]", n, e->d.max_images);
  if (group < 0) return fail(SSP2_EINVAL, "group=%d", group);
  if (total_rows(make_rowmap(e->tokens, n, group), n) > e->rows_cap) return fail(SSP2_ESTATE, "slab layout of %d images in groups of %d exceeds the workspace", n, group);
  return 0;
}

// ---- fp8 (e4m3) weight images --------------------------------------------------------------------------------------
static int quantise_mat(ssp2_engine* e, Mat& m) {
  const int ld8 = ceil_to(m.cols, 128);
  if (!m.w8 || m.ld8_cap < ld8) {
    if (dalloc(e, &m.w8, (size_t)m.rows_pad * ld8, false)) return SSP2_ENOMEM;
    m.ld8_cap = ld8;
  }
  if (!m.wscale && dalloc(e, &m.wscale, (size_t)m.rows_pad, false)) return SSP2_ENOMEM;
  m.ld8 = ld8;
  hipLaunchKernelGGL(quant_rows_e4m3_kernel, dim3((m.rows_pad + 3) / 4), dim3(256), 0, e->stream, m.w, m.ld, m.w8, ld8, m.wscale, m.rows, m.cols, m.rows_pad);
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp2_set_precision(ssp2_handle e, int mode) {
  if (!e) return fail(SSP2_EINVAL, "null handle");
  if (mode == SSP2_PREC_BF16) { e->fp8 = false; return 0; }
  if (mode != SSP2_PREC_FP8) return fail(SSP2_EINVAL, "unknown precision %d", mode);
  if (attn_streaming(e) && !e->opt[SSP2_OPT_STREAM_FP8])
    return fail(SSP2_ESTATE, "set_precision(fp8): this engine runs the key-streaming attention (SSP2_OPT_ATTN_STREAM = %d, %d tokens), which is bf16 only",
                e->opt[SSP2_OPT_ATTN_STREAM], e->tokens);
  int rc;
  for (int l = 0; l < e->d.depth; ++l) {
    Layer& L = e->layers[l];
    if (!(L.qkv.w_set && L.fc1.w_set && L.fc2.w_set)) return fail(SSP2_ESTATE, "set_precision(fp8): layer %d weights not loaded yet", l);
    if ((rc = quantise_mat(e, L.qkv)) || (rc = quantise_mat(e, L.fc1)) || (rc = quantise_mat(e, L.fc2))) return rc;
    if (L.proj.w_set && (rc = quantise_mat(e, L.proj))) return rc;       // the e4m3 out-projection (SSP2_OPT_FP8_PROJ)
  }
  if (!e->hbuf8) {
    e->ld8_dim = ceil_to(e->d.dim, 128);
    e->ld8_int_max = ceil_to(e->ld_int_max, 128);
    if ((rc = dalloc(e, &e->hbuf8, (size_t)e->rows_cap * e->ld8_dim, true))) return rc;
    if ((rc = dalloc(e, &e->act8, (size_t)e->rows_cap * e->ld8_int_max, true))) return rc;
    if ((rc = dalloc(e, &e->hscale, (size_t)e->rows_cap, true))) return rc;
    if ((rc = dalloc(e, &e->obuf8, (size_t)e->rows_cap * e->ld8_dim, true))) return rc;
    if ((rc = dalloc(e, &e->fp8_sat, 4, true))) return rc;                   // (zeroed by dalloc)
    if ((rc = dalloc(e, &e->attn_amax, (size_t)e->d.depth, true))) return rc;
    if ((rc = dalloc(e, &e->act8_top, (size_t)1, true))) return rc;
  }
  e->fp8 = true;
  return 0;
}

int ssp2_embed(ssp2_handle e, const float* pixels_dev, int n, float* x_dev, int group) {
  int rc;
  if ((rc = check_n(e, n, group))) return rc;
  const RowMap rm = make_rowmap(e->tokens, n, group);
  if (!pixels_dev || !x_dev) return fail(SSP2_EINVAL, "null device pointer");
  if (!(e->patch.w_set && e->patch.b_set && e->misc_set[0] && e->misc_set[1])) return fail(SSP2_ESTATE, "patch/cls/pos weights not loaded");
  if (e->dist && !e->dist_set) return fail(SSP2_ESTATE, "distillation token not loaded (SSP2_T_DIST)");
  if (e->reg_tokens && !e->reg_set) return fail(SSP2_ESTATE, "register tokens not loaded (ssp2_set_reg_tokens)");
  const int D = e->d.dim;
  const int pos_row0 = e->pos_prefix_rows ? e->prefix : 0;      // position row of patch 0
  if (rm.group > 0) {   // pad rows between slabs must hold finite values: they flow through LN / GEMMs (never scored).  Only THEY are
    // zeroed (one strided fill: 4.7 MB for eight 64-image ViT-B/16 slabs; round 2 cleared all 310 MB of x per stage-1 launch)
    const int n_slabs = (n + rm.group - 1) / rm.group, pad_rows = rm.mpad - rm.group * rm.tokens;
    if (n_slabs > 1 && pad_rows > 0)
      HIPCHK(hipMemset2DAsync(x_dev + (size_t)rm.group * rm.tokens * D, (size_t)rm.mpad * D * 4, 0, (size_t)pad_rows * D * 4, (size_t)(n_slabs - 1), e->stream));
  }
  {
    ProfScope ps(e, SSP2_K_OTHER);
    hipLaunchKernelGGL(cls_row_kernel, dim3((unsigned)(((long)n * e->prefix * D + 255) / 256)), dim3(256), 0, e->stream, x_dev, e->cls, e->pos, n, rm, D,
                       e->dist, e->prefix, e->reg, e->pos_prefix_rows);
    HIPCHK(hipGetLastError());
  }
  if (e->opt[SSP2_OPT_PATCH_LDS]) {
    // default: the patch tiles go pixels -> registers (bf16 rounding) -> LDS inside the GEMM kernel (patch.hip.h); the
    // im2col image (154 MB per 512 ViT-B/16 images, written and read back) does not exist
    PatchArgs a{};
    a.px = pixels_dev; a.W = e->patch.w; a.ldw = e->patch.ld; a.bias = e->patch.b; a.pos = e->pos; a.x = x_dev; a.ldx = D;
    a.n = n; a.img = e->d.img; a.p = e->d.patch; a.side = e->side; a.K = e->kpe; a.Kpad = e->kpe_pad; a.N = D;
    a.tiles_n = e->patch.rows_pad / GEMM_BN; a.rm = rm; a.prefix = e->prefix; a.pos_row0 = pos_row0;
    const int tiles_m = (n * e->patches + GEMM_BM - 1) / GEMM_BM;
    static bool attr_done[kMaxDevices] = {};
    if (!attr_done[e->dev]) {
      HIPCHK(hipFuncSetAttribute((const void*)patch_embed_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PATCH_LDS_BYTES));
      attr_done[e->dev] = true;
    }
    ProfScope ps(e, SSP2_K_GEMM_PATCH, 2.0 * n * e->patches * (double)D * e->kpe_pad);
    hipLaunchKernelGGL(patch_embed_kernel, dim3(tiles_m * a.tiles_n), dim3(256), PATCH_LDS_BYTES, e->stream, a);
    HIPCHK(hipGetLastError());
    return 0;
  }
  // SSP2_OPT_PATCH_LDS = 0 (the round-1/2 path, kept for the bit-identity test): im2col image in HBM + gemm_bf16_kernel<EPI_PATCH>
  if (!e->a_pe) {
    int rc2;
    if ((rc2 = dalloc(e, &e->a_pe, (size_t)e->d.max_images * e->patches * e->kpe_pad, true))) return rc2;
  }
  {
    ProfScope ps(e, SSP2_K_OTHER);
    const long total = (long)n * e->patches * (e->kpe_pad / 8);
    int blocks = (int)((total + 255) / 256);
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(im2col_patch_kernel, dim3(blocks), dim3(256), 0, e->stream, pixels_dev, e->a_pe, n, e->d.img,
                       e->d.patch, e->side, e->kpe, e->kpe_pad);
    HIPCHK(hipGetLastError());
  }
  GemmArgs g = bind(e->patch, act_bf16(e->a_pe, e->kpe_pad), n * e->patches, D);
  g.x = x_dev; g.ldx = D; g.pos = e->pos; g.patches = e->patches; g.prefix = e->prefix; g.pos_row0 = pos_row0; g.group = rm.group; g.mpad = rm.mpad; g.n_img = n;
  return launch_gemm<EPI_PATCH>(e, g, SSP2_K_GEMM_PATCH);
}

int ssp2_layers(ssp2_handle e, float* x, int n, int l_begin, int l_end, const uint8_t* attn_skip, int score_site,
                int score_chain, int score_group, float* batch_scores, int score_ld) {
  return ssp2_layers_from(e, nullptr, x, n, l_begin, l_end, attn_skip, score_site, score_chain, score_group, batch_scores, score_ld);
}

int ssp2_layers_from(ssp2_handle e, const float* x_in, float* x, int n, int l_begin, int l_end, const uint8_t* attn_skip, int score_site,
                     int score_chain, int score_group, float* batch_scores, int score_ld) {
  return ssp2_layers_prefix(e, x_in, x, n, l_begin, l_end, attn_skip, score_site, score_chain, score_group, n, batch_scores, score_ld);
}

// The block loop's LayerNorm output lives in hbuf (bf16) or, for a projection on e4m3 operands, in hbuf8 + hscale (e4m3 bytes, one scale
// per row).  Three things must agree on that: the standalone LayerNorm that writes it, the LayerNorm fused behind a residual GEMM (lab
// build) that writes it instead, and the operand the next projection binds.
static int ln_to_hbuf(ssp2_engine* e, const float* x, const float* gm, const float* bt, int M, bool fp8, bool* h_ready) {
  const int D = e->d.dim;
  if (*h_ready) { *h_ready = false; return 0; }      // a residual GEMM has written it already: the hand-off is used up
  return fp8 ? launch_ln(e, x, D, gm, bt, nullptr, e->ld8_dim, M, D, RowMap{0, 0, 0}, e->hbuf8, e->hscale) : launch_ln(e, x, D, gm, bt, e->hbuf, D, M, D);
}
static void fuse_ln_to_hbuf(const ssp2_engine* e, GemmArgs& a, const float* gm, const float* bt, bool fp8) {
  a.ln_g = gm; a.ln_b = bt; a.ln_eps = e->d.ln_eps;
  if (fp8) { a.ln_out8 = e->hbuf8; a.ln_ld = e->ld8_dim; a.ln_ascale = e->hscale; } else { a.ln_out = e->hbuf; a.ln_ld = e->d.dim; }
}
static ActOperand hbuf_operand(const ssp2_engine* e, bool fp8) { return fp8 ? act_e4m3(e->hbuf8, e->ld8_dim, e->hscale) : act_bf16(e->hbuf, e->d.dim); }

// One ssp2_layers_prefix call: what its argument checks derive, and (last line) the two things that change from block to block
struct LayersCall {
  float* x; const uint8_t* attn_skip; int l_end;
  int n, M; RowMap rm;                        // images and token-matrix rows of the launch
  int score_site, score_chain; bool scores_only; float* batch_scores; int score_ld;
  bool fused;                                 // the fc1 epilogue scores (a 128-row tile then spans at most two samples); else the standalone L2 kernel
  bool split; int ns, M0;                     // hook on the leading ns images only: fc1 runs as rows [0, M0) scored + rows [M0, M) plain
  int grp; size_t group_stride;               // score groups of the hooked images
  // fp8 mode: the three large projections of a launch with >= 4096 rows run on e4m3 operands (LayerNorm and the fc1
  // epilogue write the activation as e4m3 bytes); attention, the out-projection and small launches stay bf16
  bool f8, f8_fc1;
  // xsrc: where the residual stream is READ — x_in for the block the call enters with (LayerNorm input and the first residual add),
  // x from the first residual add on (out of place for one residual epilogue, no copy of the stream)
  // h_ready: hbuf / hbuf8 already holds the LayerNorm the next projection reads (written by a residual GEMM)
  const float* xsrc; bool h_ready;
};
static inline bool attn_skipped(const ssp2_engine* e, const LayersCall& c, int l) { return e->layers[l].attn_dropped || (c.attn_skip && c.attn_skip[l]); }

// The attention half of block l: LN1, QKV, attention, out-projection + residual
static int attn_half(ssp2_engine* e, LayersCall& c, int l) {
  int rc;
  Layer& L = e->layers[l];
  const int D = e->d.dim, M = c.M;
  if ((rc = ln_to_hbuf(e, c.xsrc, L.ln1_g, L.ln1_b, M, c.f8, &c.h_ready))) return rc;
  GemmArgs q = bind(L.qkv, hbuf_operand(e, c.f8), M, 3 * D);
  q.out = e->qkvbuf; q.ldo = 3 * D;
  if ((rc = dispatch_gemm(e, EPI_BF16, c.f8, q, SSP2_K_GEMM_QKV))) return rc;
  // fp8 out-projection (SSP2_OPT_FP8_PROJ): the persistent attention kernel (or, SSP2_OPT_STREAM_FP8, the key-streaming one) writes
  // e4m3(o * 16) bytes, the projection runs on e4m3 operands and divides the 16 out in its epilogue
  // (during ssp2_fp8_calibrate_* the projection stays on bf16 and the block's max |o| is recorded)
  const bool f8_proj = c.f8 && e->opt[SSP2_OPT_FP8_PROJ] && attn_writes_e4m3(e) && has_e4m3(L.proj) && D % 64 == 0 && !e->fp8_calibrating;
  if ((rc = launch_attn(e, c.n, c.rm, false, f8_proj ? e->obuf8 : nullptr, L.o8_scale))) return rc;
  if (c.f8 && e->fp8_calibrating && e->attn_amax) {
    ProfScope ps(e, SSP2_K_OTHER);
    hipLaunchKernelGGL(absmax_bf16_kernel, dim3(1024), dim3(256), 0, e->stream, e->obuf, (long)M, D, D, e->attn_amax + l, c.rm, c.n);
    HIPCHK(hipGetLastError());
  }
  GemmArgs p = bind(L.proj, f8_proj ? act_e4m3(e->obuf8, e->ld8_dim, nullptr, 1.0f / L.o8_scale) : act_bf16(e->obuf, D), M, D);
  p.x = c.x; p.ldx = D; p.xin = c.xsrc;
  // a branch with LayerScale takes the product form only: the lab forms (LayerNorm behind the epilogue, deferred residual) know no scale
  const int epi = resid_epi(L, 0, p);
  const int lnv = epi == EPI_RESID ? ln_fusable(e, M, D, f8_proj) : 0;        // + LN2 of this layer: fc1's operand
  if (lnv) fuse_ln_to_hbuf(e, p, L.ln2_g, L.ln2_b, c.f8_fc1);
  if ((rc = dispatch_gemm(e, epi, f8_proj, p, SSP2_K_GEMM_PROJ, lnv))) return rc;
  c.h_ready = lnv != 0;
  c.xsrc = c.x;
  return 0;
}

// The stage-1 hook of block l: the hooked images' activation norms, summed per score group into the block's row of batch_scores
static int score_finish(ssp2_engine* e, const LayersCall& c, int l) {
  const Layer& L = e->layers[l];
  float* row = c.batch_scores + (size_t)l * c.score_ld;
  if (c.fused) {
    ProfScope ps(e, SSP2_K_SCORE_FINISH);
    return score_finish_fused(e->stream, e->slab, c.ns, c.rm, c.grp, L.ld_int, c.score_chain, e->norms, row, c.group_stride);
  }
  const bf16* seen = (c.score_site == SSP2_SCORE_PRE_GELU) ? e->prebuf : e->actbuf;
  ProfScope ps(e, SSP2_K_ACT_L2);
  return act_l2_impl(e->stream, seen, 0, c.ns, c.rm, L.d_int, L.ld_int, c.score_chain, c.grp, e->norms, row, c.group_stride);
}

// The MLP half of block l: LN2, fc1 + GELU (with the scoring epilogue where the call hooks it), the score finish, fc2 + residual
static int mlp_half(ssp2_engine* e, LayersCall& c, int l) {
  int rc = 0;
  Layer& L = e->layers[l];
  const int D = e->d.dim, M = c.M;
  const bool f8 = c.f8_fc1;                      // fc1 and fc2 of a block share a format: the activation between them is e4m3 bytes or bf16
  const int ld8_int = ceil_to(L.ld_int, 128);
  if ((rc = ln_to_hbuf(e, c.xsrc, L.ln2_g, L.ln2_b, M, f8, &c.h_ready))) return rc;
  GemmArgs f = bind(L.fc1, hbuf_operand(e, f8), M, f8 ? ld8_int : L.ld_int);
  if (f8) { f.out = (bf16*)e->act8; f.ldo = ld8_int; }      // e4m3 bytes out; the pad columns up to 128 are written (zeros)
  else { f.out = e->actbuf; f.ldo = L.ld_int; }
  f.score_site = c.fused ? c.score_site : 0; f.tokens = e->tokens; f.slab = e->slab; f.slab_ld = L.ld_int;
  f.group = c.rm.group; f.mpad = c.rm.mpad; f.n_img = c.ns;
  f.group_m = 8;   // 8 x 8 tile patches per XCD: the 4.7 MB fc1 weight no longer thrashes the 4 MiB L2 (PMC: FETCH_SIZE / 3.7)
  // unfused pre-GELU scoring (models with < 128 tokens): the hook sees fc1's output, fc2 consumes the GELU
  // of it, so the epilogue also stores the pre-activation for the standalone L2 kernel to read.
  f.out2 = (c.score_site == SSP2_SCORE_PRE_GELU && !c.fused) ? e->prebuf : nullptr;
  if (c.split && c.fused) {
    // the hooked slabs with the scoring epilogue, the rest of the launch (the search's candidates) without it
    // (one operation as far as the zigzag goes: both launches walk in the direction the whole launch would have taken, the part
    // that direction meets first goes first)
    GemmArgs r = gemm_rows_from(f, c.M0);
    r.score_site = 0; r.n_img = c.n - c.ns;
    f.M = c.M0;
    const int dir = next_dir(e);
    e->zig_hold = dir;
    if (!dir) rc = dispatch_gemm(e, EPI_FC1, f8, f, SSP2_K_GEMM_FC1);
    if (!rc) rc = dispatch_gemm(e, EPI_FC1, f8, r, SSP2_K_GEMM_FC1);
    if (!rc && dir) rc = dispatch_gemm(e, EPI_FC1, f8, f, SSP2_K_GEMM_FC1);
    e->zig_hold = -1;                             // (on the error paths too)
  } else {
    rc = dispatch_gemm(e, EPI_FC1, f8, f, SSP2_K_GEMM_FC1);
  }
  if (rc) return rc;
  if (f8 && e->fp8_calibrating && e->act8_top) {       // calibration pass: how much of the GELU output did the saturating e4m3 cast put on its top code?
    ProfScope ps(e, SSP2_K_OTHER);
    hipLaunchKernelGGL(e4m3_top_code_count_kernel, dim3(1024), dim3(256), 0, e->stream, e->act8, (long)M, ceil_to(L.d_int, 16), ld8_int, e->act8_top, c.rm, c.n);
    HIPCHK(hipGetLastError());
  }
  if (c.score_site && (rc = score_finish(e, c, l))) return rc;
  if (c.scores_only && l + 1 == c.l_end) return 0;            // nothing reads x behind the last hooked activation
  GemmArgs o = bind(L.fc2, f8 ? act_e4m3(e->act8, ld8_int, nullptr) : act_bf16(e->actbuf, L.ld_int), M, D);
  o.x = c.x; o.ldx = D; o.xin = c.xsrc;
  const int epi = resid_epi(L, 1, o);
  // + the LayerNorm the NEXT layer of this call starts with: LN1 of layer l + 1, or its LN2 when its attention is skipped
  // (not behind a LayerScale epilogue: product form only)
  int lnv = 0;
  if (l + 1 < c.l_end && epi == EPI_RESID) {
    const Layer& Ln = e->layers[l + 1];
    const bool skip_n = attn_skipped(e, c, l + 1);
    if (skip_n ? (Ln.ln_set[2] && Ln.ln_set[3]) : (Ln.ln_set[0] && Ln.ln_set[1])) {
      lnv = ln_fusable(e, M, f8 ? ld8_int : L.ld_int, f8);
      if (lnv) fuse_ln_to_hbuf(e, o, skip_n ? Ln.ln2_g : Ln.ln1_g, skip_n ? Ln.ln2_b : Ln.ln1_b, skip_n ? c.f8_fc1 : c.f8);
    }
  }
  if ((rc = dispatch_gemm(e, epi, f8, o, SSP2_K_GEMM_FC2, lnv))) return rc;
  c.h_ready = lnv != 0;
  c.xsrc = c.x;
  return 0;
}

// score_images < n: only the LEADING score_images images of the launch are hooked (whole slabs of the slab layout).  This is the depth
// search's baseline doubling as the stage-1 pass (reference: ONE loader and ONE batch_limit feed both stages,
// adaptation-for-Pures-framework/mask_conjunction.py:276-281, :327): slot 0 of the layer-major launch is scored, the candidates' slots
// behind it are not.  Only the fc1 GEMM is split in two launches at the (128-row aligned) slab boundary; a row's arithmetic does not
// depend on the launch it is part of, so the stream and the scores are the bits of a scored launch of score_images images alone.
int ssp2_layers_prefix(ssp2_handle e, const float* x_in, float* x, int n, int l_begin, int l_end, const uint8_t* attn_skip, int score_site,
                       int score_chain, int score_group, int score_images, float* batch_scores, int score_ld) {
  int rc;
  if ((rc = check_n(e, n, score_group))) return rc;
  if (score_images <= 0 || score_images > n) return fail(SSP2_EINVAL, "score_images=%d outside (0, n=%d]", score_images, n);
  if (!x) return fail(SSP2_EINVAL, "null x");
  if (l_begin < 0 || l_end > e->d.depth || l_begin > l_end) return fail(SSP2_EINVAL, "bad layer range [%d,%d)", l_begin, l_end);
  LayersCall c{};
  c.scores_only = (score_site & SSP2_SCORE_ONLY) != 0;
  score_site &= ~SSP2_SCORE_ONLY;
  if (score_site < 0 || score_site > 2) return fail(SSP2_EINVAL, "bad score_site %d", score_site);
  if (c.scores_only && !score_site) return fail(SSP2_EINVAL, "SSP2_SCORE_ONLY without a score site");
  if (score_site && (!batch_scores || score_ld < e->ld_int_max)) return fail(SSP2_EINVAL, "batch_scores needs ld >= %d", e->ld_int_max);
  c.x = x; c.attn_skip = attn_skip; c.l_end = l_end;
  c.n = n; c.rm = make_rowmap(e->tokens, n, score_group); c.M = (int)total_rows(c.rm, n);
  c.score_site = score_site; c.score_chain = score_chain; c.batch_scores = batch_scores; c.score_ld = score_ld;
  c.split = score_site && score_images < n;
  if (c.split && (c.rm.group <= 0 || score_images % c.rm.group != 0 || c.scores_only))
    return fail(SSP2_EINVAL, "score_images=%d < n=%d needs the slab layout, whole slabs (group %d) and no SSP2_SCORE_ONLY", score_images, n, score_group);
  c.ns = score_site ? score_images : n;                                            // images that are hooked
  c.M0 = c.split ? (score_images / c.rm.group) * c.rm.mpad : c.M;                  // rows of the scored prefix: whole padded slabs
  c.grp = (score_group <= 0 || score_group > n) ? n : score_group;
  c.group_stride = (size_t)e->d.depth * score_ld;
  c.fused = score_site && e->tokens >= GEMM_BM;
  c.f8 = e->fp8 && c.M >= big_tile_min_rows(e);
  c.f8_fc1 = c.f8 && fused_ok_for_fp8(score_site, e->tokens);
  c.xsrc = (x_in && x_in != x) ? x_in : x;
  for (int l = l_begin; l < l_end; ++l) {
    const Layer& L = e->layers[l];
    if (!mlp_loaded(L)) return fail(SSP2_ESTATE, "layer %d MLP weights not loaded", l);
    if (!attn_skipped(e, c, l)) {
      if (!attn_loaded(L)) return fail(SSP2_ESTATE, "layer %d attention weights not loaded", l);
      if ((rc = attn_half(e, c, l))) return rc;
    }
    if ((rc = mlp_half(e, c, l))) return rc;
  }
  return 0;
}

// The head on the rows it reads: row 0 of every image (CLS), and row 1 (DIST) too with the distillation head.  x holds them either
// where ssp2_embed put them (prefix_major = false: image r's prefix row t at x + t * D + r * in_stride, or through the row map `gather`),
// or already compacted prefix-major [tail_rows][n][D] at a row stride of in_stride (prefix_major = true: the tail's x_cls).
static int head_impl(ssp2_engine* e, const float* x, size_t in_stride, int n, float* logits_dev, int32_t* pred, const int64_t* labels,
                     int64_t* correct, RowMap gather = RowMap{0, 0, 0}, int period = 0, bool prefix_major = false) {
  int rc;
  if (!(e->misc_set[2] && e->misc_set[3] && e->head.w_set && e->head.b_set)) return fail(SSP2_ESTATE, "final norm / head weights not loaded");
  if (e->dist_head && !(e->head_dist.w_set && e->head_dist.b_set)) return fail(SSP2_ESTATE, "distillation head weights not loaded");
  const int D = e->d.dim, C = e->d.classes, hr = e->tail_rows;
  if (prefix_major) {
    if ((rc = launch_ln(e, x, in_stride, e->lnf_g, e->lnf_b, e->cls_h, D, hr * n, D, gather))) return rc;
  } else {
    for (int t = 0; t < hr; ++t)
      if ((rc = launch_ln(e, x + (size_t)t * D, in_stride, e->lnf_g, e->lnf_b, e->cls_h + (size_t)t * n * D, D, n, D, gather))) return rc;
  }
  float* lg = e->dist_head ? e->logits : (logits_dev ? logits_dev : e->logits);
  GemmArgs g = bind(e->head, act_bf16(e->cls_h, D), n, C);
  g.x = lg; g.ldx = C;
  if ((rc = launch_gemm<EPI_F32>(e, g, SSP2_K_GEMM_HEAD))) return rc;
  if (e->dist_head) {   // head_dist on the DIST rows, then logits = 0.5f * bf16(a + b) (autocast's rounding points) and the top-1 of the mean in one kernel
    float* lb = e->logits + (size_t)n * C;
    float* out = logits_dev ? logits_dev : e->logits + (size_t)2 * n * C;
    GemmArgs h = bind(e->head_dist, act_bf16(e->cls_h + (size_t)n * D, D), n, C);
    h.x = lb; h.ldx = C;
    if ((rc = launch_gemm<EPI_F32>(e, h, SSP2_K_GEMM_HEAD))) return rc;
    ProfScope ps(e, SSP2_K_OTHER);
    hipLaunchKernelGGL(dist_head_top1_kernel, dim3((n + 3) / 4), dim3(256), 0, e->stream, lg, lb, out, n, C, pred, labels,
                       (unsigned long long*)correct, period);
    HIPCHK(hipGetLastError());
    return 0;
  }
  if (pred || (labels && correct)) {
    ProfScope ps(e, SSP2_K_OTHER);
    hipLaunchKernelGGL(argmax_top1_kernel, dim3((n + 3) / 4), dim3(256), 0, e->stream, lg, n, C, pred, labels,
                       (unsigned long long*)correct, period);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

int ssp2_head(ssp2_handle e, const float* x, int n, int group, float* logits_dev, int32_t* pred, const int64_t* labels, int64_t* correct) {
  int rc;
  if ((rc = check_n(e, n, group))) return rc;
  if (!x) return fail(SSP2_EINVAL, "null x");
  return head_impl(e, x, (size_t)e->tokens * e->d.dim, n, logits_dev, pred, labels, correct, make_rowmap(e->tokens, n, group));
}

int ssp2_tail(ssp2_handle e, const float* x, int n, int attn_skip_last, float* logits_dev, int32_t* pred, const int64_t* labels,
              int64_t* correct) {
  return ssp2_tail_slots(e, x, n, 1, attn_skip_last, logits_dev, pred, labels, correct);
}

// The tail over `slots` residual streams of n_slot images each, laid side by side in x (slot s = rows [s * n_slot * tokens,
// (s + 1) * n_slot * tokens)) — the baseline and the candidates of the layer-major search, which all meet the SAME last block
// and classifier.  One launch sequence for slots * n_slot images instead of one per slot: the tail's launches on n_slot CLS rows
// (two LayerNorms, q / out-projection / fc1 / fc2 on 320 rows, CLS attention, head, argmax: ~10 kernels of 10-40 us each,
// latency-bound) were 13 x ~0.25 ms of a 108 ms step.  Per image the arithmetic is unchanged (no result of a row depends on
// how many rows a launch has), so the counts are the same integers.  labels [n_slot] is shared by the slots, correct [slots].
int ssp2_tail_slots(ssp2_handle e, const float* x, int n_slot, int slots, int attn_skip_last, float* logits_dev, int32_t* pred,
                    const int64_t* labels, int64_t* correct) {
  return ssp2_tail_group(e, x, n_slot, slots, 0, attn_skip_last, logits_dev, pred, labels, correct);
}

// ... and with the streams in the SLAB layout (group > 0: slabs of `group` images, ssp2_rows; n_slot a multiple of group, so that slot s
// starts at slab s * n_slot / group): the tail of the search whose baseline doubles as the stage-1 pass (ssp2_layers_prefix).  Pad rows
// between the slabs take part in the row-wise kernels (LayerNorm, the key / value projection) and are read by nobody.
int ssp2_tail_group(ssp2_handle e, const float* x, int n_slot, int slots, int group, int attn_skip_last, float* logits_dev, int32_t* pred,
                    const int64_t* labels, int64_t* correct) {
  int rc;
  if (slots <= 0 || n_slot <= 0) return fail(SSP2_EINVAL, "tail: n_slot=%d slots=%d", n_slot, slots);
  const int n = n_slot * slots;
  const int period = slots > 1 ? n_slot : 0;
  if ((rc = check_n(e, n, group))) return rc;
  if (!x) return fail(SSP2_EINVAL, "null x");
  const RowMap rm = make_rowmap(e->tokens, n, group);
  if (rm.group > 0 && slots > 1 && n_slot % rm.group != 0) return fail(SSP2_EINVAL, "tail: slots of %d images are not whole slabs of %d", n_slot, group);
  const int D = e->d.dim, M = (int)total_rows(rm, n), l = e->d.depth - 1;
  const int P = e->tail_rows, PN = P * n;              // rows the tail carries: CLS, and DIST with the distillation head
  Layer& L = e->layers[l];
  if (!mlp_loaded(L)) return fail(SSP2_ESTATE, "last layer MLP weights not loaded");
  // x_cls <- prefix rows 0..P-1 of x, prefix-major [P][n][D] (x itself is left untouched)
  if (rm.group > 0) {
    ProfScope ps(e, SSP2_K_OTHER);
    hipLaunchKernelGGL(gather_cls_rows_kernel, dim3((unsigned)(((long)PN * (D / 4) + 255) / 256)), dim3(256), 0, e->stream, x, e->x_cls, n, rm, D, P);
    HIPCHK(hipGetLastError());
  } else {
    for (int t = 0; t < P; ++t)
      HIPCHK(hipMemcpy2DAsync(e->x_cls + (size_t)t * n * D, (size_t)D * 4, x + (size_t)t * D, (size_t)e->tokens * D * 4, (size_t)D * 4, n,
                              hipMemcpyDeviceToDevice, e->stream));
  }
  if (!attn_skip_last && !L.attn_dropped) {
    if (!attn_loaded(L)) return fail(SSP2_ESTATE, "last layer attention weights not loaded");
    // keys / values need every token; the query, the out-projection and the MLP only the P prefix rows
    if ((rc = launch_ln(e, x, D, L.ln1_g, L.ln1_b, e->hbuf, D, M, D))) return rc;
    GemmArgs kv = bind_rows(L.qkv, D, act_bf16(e->hbuf, D), M, 2 * D);            // weight rows [D, 3 D): keys and values
    kv.out = e->qkvbuf + D; kv.ldo = 3 * D;
    if ((rc = dispatch_gemm(e, EPI_BF16, false, kv, SSP2_K_GEMM_QKV))) return rc;
    if ((rc = launch_ln(e, e->x_cls, D, L.ln1_g, L.ln1_b, e->h_cls, D, PN, D))) return rc;     // the same rows' bits as the full LN1
    GemmArgs q = bind_rows(L.qkv, 0, act_bf16(e->h_cls, D), PN, D);               // weight rows [0, D): the queries
    q.out = e->q_cls; q.ldo = D;
    if ((rc = dispatch_gemm(e, EPI_BF16, false, q, SSP2_K_GEMM_QKV))) return rc;
    if ((rc = launch_attn(e, n, rm, true))) return rc;
    GemmArgs p = bind(L.proj, act_bf16(e->o_cls, D), PN, D);
    p.x = e->x_cls; p.ldx = D;
    if ((rc = dispatch_gemm(e, resid_epi(L, 0, p), false, p, SSP2_K_GEMM_PROJ))) return rc;
  }
  if ((rc = launch_ln(e, e->x_cls, D, L.ln2_g, L.ln2_b, e->h_cls, D, PN, D))) return rc;
  GemmArgs f = bind(L.fc1, act_bf16(e->h_cls, D), PN, L.ld_int);
  f.out = e->act_cls; f.ldo = L.ld_int;
  if ((rc = dispatch_gemm(e, EPI_FC1, false, f, SSP2_K_GEMM_FC1))) return rc;
  GemmArgs o = bind(L.fc2, act_bf16(e->act_cls, L.ld_int), PN, D);
  o.x = e->x_cls; o.ldx = D;
  if ((rc = dispatch_gemm(e, resid_epi(L, 1, o), false, o, SSP2_K_GEMM_FC2))) return rc;
  return head_impl(e, e->x_cls, (size_t)D, n, logits_dev, pred, labels, correct, RowMap{0, 0, 0}, period, true);
}

int ssp2_d_int(ssp2_handle e, int layer) {
  if (!e || layer < 0 || layer >= e->d.depth) return fail(SSP2_EINVAL, "bad layer");
  return e->layers[layer].d_int;
}

int ssp2_drop_attention(ssp2_handle e, int layer) {
  if (!e || layer < 0 || layer >= e->d.depth) return fail(SSP2_EINVAL, "bad layer");
  e->layers[layer].attn_dropped = true;
  return 0;
}

// Host keep list -> device, without relying on the caller's buffer after return.  hipMemcpyAsync stages PAGEABLE sources before it
// returns, but a PINNED source (hipHostMalloc, torch pin_memory) is read by the DMA engine whenever the stream gets there — the
// caller may have freed or rewritten the list by then.  The list is therefore copied (host memcpy, <= 20 KB) into the engine's own
// pinned slot of that layer first; a slot is re-used only by the next prune of the SAME layer, whose event wait is a no-op unless
// that earlier copy is still queued.
static int stage_keep(ssp2_engine* e, int layer, const int32_t* keep, int n_keep, int* dev_dst, hipStream_t stream) {
  const size_t slot = (size_t)std::max(e->ld_int_max, 64);
  if (!e->keep_pin) {
    HIPCHK(hipHostMalloc((void**)&e->keep_pin, slot * e->d.depth * sizeof(int32_t)));
    e->keep_pin_slot = slot;
    e->keep_ev.assign(e->d.depth, nullptr);
    e->keep_ev_set.assign(e->d.depth, 0);
    for (auto& ev : e->keep_ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  }
  if ((size_t)n_keep > e->keep_pin_slot) return fail(SSP2_EINVAL, "keep list of %d entries exceeds the widest block (%zu)", n_keep, e->keep_pin_slot);
  if (e->keep_ev_set[layer]) HIPCHK(hipEventSynchronize(e->keep_ev[layer]));
  int32_t* pin = e->keep_pin + (size_t)layer * e->keep_pin_slot;
  memcpy(pin, keep, (size_t)n_keep * sizeof(int32_t));
  HIPCHK(hipMemcpyAsync(dev_dst, pin, (size_t)n_keep * 4, hipMemcpyHostToDevice, stream));
  HIPCHK(hipEventRecord(e->keep_ev[layer], stream));
  e->keep_ev_set[layer] = 1;
  return 0;
}

int ssp2_prune_ffn(ssp2_handle e, int layer, const int32_t* keep, int n_keep) {
  if (!e || !keep || layer < 0 || layer >= e->d.depth) return fail(SSP2_EINVAL, "bad argument");
  Layer& L = e->layers[layer];
  if (n_keep <= 0 || n_keep > L.d_int) return fail(SSP2_EINVAL, "n_keep=%d outside (0, d_int=%d]", n_keep, L.d_int);
  for (int i = 0; i < n_keep; ++i)
    if (keep[i] < 0 || keep[i] >= L.d_int || (i && keep[i] <= keep[i - 1])) return fail(SSP2_EINVAL, "keep list must be ascending and inside [0, d_int)");
  if (!(L.fc1.w_set && L.fc1.b_set && L.fc2.w_set)) return fail(SSP2_ESTATE, "layer %d MLP weights not loaded", layer);
  const int D = e->d.dim;
  const int new_ld = ceil_to(n_keep, GEMM_BK);
  const size_t fc1_elems = (size_t)L.fc1.rows_pad * L.fc1.ld, fc2_elems = (size_t)L.fc2.rows_pad * new_ld;
  // Scratch of the in-place gather lives in the engine: allocated at the first call for the WIDEST block (every later call,
  // on any layer, fits), so a prune is stream-ordered device work — no hipMalloc / hipFree, no stream synchronisation
  // (round 2: four of each per block and two synchronisations).  The keep list crosses PCIe out of the engine's own pinned slot
  // (stage_keep): the caller's buffer is not read after return, pageable or pinned.
  auto grow = [&](auto** p, size_t& cap, size_t want, size_t worst) -> int {
    if (cap >= want) return 0;
    HIPCHK(hipStreamSynchronize(e->stream));        // (only when a buffer must be replaced: work in flight may still read it)
    if (*p) hipFree(*p);
    *p = nullptr; cap = 0;
    const size_t n = std::max(want, worst);
    HIPCHK(hipMalloc((void**)p, n * sizeof(**p)));
    cap = n;
    return 0;
  };
  size_t worst1 = 0, worst2 = 0, worstb = 0, worstk = 0;
  for (const Layer& Lx : e->layers) {
    worst1 = std::max(worst1, (size_t)Lx.fc1.rows_pad * Lx.fc1.ld); worst2 = std::max(worst2, (size_t)Lx.fc2.rows_pad * Lx.fc2.ld);
    worstb = std::max(worstb, (size_t)Lx.fc1.rows_pad); worstk = std::max(worstk, (size_t)Lx.d_int);
  }
  int rc0;
  if ((rc0 = grow(&e->prune_t1, e->prune_t1_cap, fc1_elems, worst1)) || (rc0 = grow(&e->prune_t2, e->prune_t2_cap, fc2_elems, worst2)) ||
      (rc0 = grow(&e->prune_tb, e->prune_tb_cap, (size_t)L.fc1.rows_pad, worstb)) || (rc0 = grow(&e->prune_keep, e->prune_keep_cap, (size_t)n_keep, worstk)))
    return rc0;
  int* const keep_dev = e->prune_keep;
  bf16 *const t1 = e->prune_t1, *const t2 = e->prune_t2;
  float* const tb = e->prune_tb;
  { int rck; if ((rck = stage_keep(e, layer, keep, n_keep, keep_dev, e->stream))) return rck; }
  // fc1: rows gathered, same leading dimension (K = dim); fc2: columns gathered into the new, smaller leading dimension
  hipLaunchKernelGGL(gather_matrix_kernel, dim3(2048), dim3(256), 0, e->stream, L.fc1.w, L.fc1.ld, t1, L.fc1.ld, L.fc1.rows_pad, n_keep, D, keep_dev, (const int*)nullptr);
  hipLaunchKernelGGL(gather_vector_kernel, dim3((L.fc1.rows_pad + 255) / 256), dim3(256), 0, e->stream, L.fc1.b, tb, L.fc1.rows_pad, n_keep, keep_dev);
  hipLaunchKernelGGL(gather_matrix_kernel, dim3(2048), dim3(256), 0, e->stream, L.fc2.w, L.fc2.ld, t2, new_ld, L.fc2.rows_pad, D, n_keep, (const int*)nullptr, keep_dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(L.fc1.w, t1, fc1_elems * 2, hipMemcpyDeviceToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(L.fc1.b, tb, (size_t)L.fc1.rows_pad * 4, hipMemcpyDeviceToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(L.fc2.w, t2, fc2_elems * 2, hipMemcpyDeviceToDevice, e->stream));
  L.d_int = n_keep; L.ld_int = new_ld;
  L.fc1.rows = n_keep; L.fc2.cols = n_keep; L.fc2.ld = new_ld;
  e->d_int[layer] = n_keep;
  if (e->fp8) {                                  // fresh e4m3 images (and row scales) of the compacted matrices
    int rc;
    if ((rc = quantise_mat(e, L.fc1)) || (rc = quantise_mat(e, L.fc2))) return rc;
  }
  return 0;
}

int ssp2_restore_attention(ssp2_handle e, int layer) {
  if (!e || layer < 0 || layer >= e->d.depth) return fail(SSP2_EINVAL, "bad layer");
  e->layers[layer].attn_dropped = false;
  return 0;
}

static int copy_mat(ssp2_engine* dst, Mat& d, const Mat& s) {
  if (d.rows_pad != s.rows_pad || d.ld != s.ld) return fail(SSP2_EINVAL, "clone: matrix shapes differ (%d x %d vs %d x %d)", d.rows_pad, d.ld, s.rows_pad, s.ld);
  HIPCHK(hipMemcpyAsync(d.w, s.w, (size_t)d.rows_pad * d.ld * 2, hipMemcpyDeviceToDevice, dst->stream));
  HIPCHK(hipMemcpyAsync(d.b, s.b, (size_t)d.rows_pad * 4, hipMemcpyDeviceToDevice, dst->stream));
  d.w_set = s.w_set; d.b_set = s.b_set;
  return 0;
}

int ssp2_clone_weights(ssp2_handle dst, ssp2_handle src) {
  if (!dst || !src) return fail(SSP2_EINVAL, "null handle");
  const ssp2_vit_desc &a = dst->d, &b = src->d;
  if (a.img != b.img || a.patch != b.patch || a.dim != b.dim || a.heads != b.heads || a.depth != b.depth || a.classes != b.classes)
    return fail(SSP2_EINVAL, "clone: the two engines describe different architectures");
  if (dst->prefix != src->prefix || dst->dist_head != src->dist_head)
    return fail(SSP2_EINVAL, "clone: token layouts differ (prefix_tokens %d / %d, dist_head %d / %d)", dst->prefix, src->prefix, dst->dist_head, src->dist_head);
  if (dst->reg_tokens != src->reg_tokens || dst->pos_prefix_rows != src->pos_prefix_rows)
    return fail(SSP2_EINVAL, "clone: token layouts differ (reg_tokens %d / %d, pos_prefix_rows %d / %d)", dst->reg_tokens, src->reg_tokens,
                dst->pos_prefix_rows, src->pos_prefix_rows);
  const int D = a.dim;
  int rc;
  auto cp = [&](float* d, const float* s, size_t n) -> int { HIPCHK(hipMemcpyAsync(d, s, n * 4, hipMemcpyDeviceToDevice, dst->stream)); return 0; };
  if ((rc = copy_mat(dst, dst->patch, src->patch)) || (rc = copy_mat(dst, dst->head, src->head))) return rc;
  if ((rc = cp(dst->cls, src->cls, D)) || (rc = cp(dst->pos, src->pos, dst->pos_rows() * D)) || (rc = cp(dst->lnf_g, src->lnf_g, D)) || (rc = cp(dst->lnf_b, src->lnf_b, D))) return rc;
  for (int i = 0; i < 4; ++i) dst->misc_set[i] = src->misc_set[i];
  if (src->dist) { if ((rc = cp(dst->dist, src->dist, D))) return rc; dst->dist_set = src->dist_set; }
  if (src->reg) { if ((rc = cp(dst->reg, src->reg, (size_t)src->reg_tokens * D))) return rc; dst->reg_set = src->reg_set; }
  if (src->dist_head && (rc = copy_mat(dst, dst->head_dist, src->head_dist))) return rc;
  for (int l = 0; l < a.depth; ++l) {
    Layer &d = dst->layers[l]; const Layer& s = src->layers[l];
    if ((rc = cp(d.ln1_g, s.ln1_g, D)) || (rc = cp(d.ln1_b, s.ln1_b, D)) || (rc = cp(d.ln2_g, s.ln2_g, D)) || (rc = cp(d.ln2_b, s.ln2_b, D))) return rc;
    for (int i = 0; i < 4; ++i) d.ln_set[i] = s.ln_set[i];
    if ((rc = copy_mat(dst, d.qkv, s.qkv)) || (rc = copy_mat(dst, d.proj, s.proj))) return rc;
    d.attn_dropped = s.attn_dropped;
    d.o8_scale = s.o8_scale;
    for (int br = 0; br < 2; ++br) {      // LayerScale is per hidden column: width pruning leaves it alone
      if (s.ls_set[br]) { if ((rc = set_layer_scale_impl(dst, d, br, s.ls[br], true))) return rc; }
      else d.ls_set[br] = false;
    }
    if (d.d_int == s.d_int) { if ((rc = copy_mat(dst, d.fc1, s.fc1)) || (rc = copy_mat(dst, d.fc2, s.fc2))) return rc; }
    else {   // the FFN arrives through ssp2_prune_ffn_into; fc2's bias does not depend on the kept neurons
      HIPCHK(hipMemcpyAsync(d.fc2.b, s.fc2.b, (size_t)d.fc2.rows_pad * 4, hipMemcpyDeviceToDevice, dst->stream));
      d.fc2.b_set = s.fc2.b_set;
    }
  }
  return 0;
}

int ssp2_prune_ffn_into(ssp2_handle dst, ssp2_handle src, int layer, const int32_t* keep, int n_keep) {
  if (!dst || !src || !keep || layer < 0 || layer >= src->d.depth || layer >= dst->d.depth) return fail(SSP2_EINVAL, "bad argument");
  Layer& S = src->layers[layer]; Layer& T = dst->layers[layer];
  if (dst->d.dim != src->d.dim) return fail(SSP2_EINVAL, "prune_ffn_into: hidden sizes differ");
  if (n_keep != T.d_int) return fail(SSP2_EINVAL, "prune_ffn_into: destination block %d is %d wide, keep list has %d entries", layer, T.d_int, n_keep);
  if (n_keep > S.d_int) return fail(SSP2_EINVAL, "n_keep=%d > source d_int=%d", n_keep, S.d_int);
  for (int i = 0; i < n_keep; ++i)
    if (keep[i] < 0 || keep[i] >= S.d_int || (i && keep[i] <= keep[i - 1])) return fail(SSP2_EINVAL, "keep list must be ascending and inside [0, d_int)");
  if (!(S.fc1.w_set && S.fc1.b_set && S.fc2.w_set)) return fail(SSP2_ESTATE, "layer %d MLP weights not loaded", layer);
  const int D = src->d.dim;
  if (!T.keep_dev) { HIPCHK(hipMalloc((void**)&T.keep_dev, (size_t)T.ld_int * 4)); dst->allocs.push_back(T.keep_dev); }
  { int rck; if ((rck = stage_keep(dst, layer, keep, n_keep, T.keep_dev, dst->stream))) return rck; }    // the caller's list may go away on return
  hipLaunchKernelGGL(gather_matrix_kernel, dim3(2048), dim3(256), 0, dst->stream, S.fc1.w, S.fc1.ld, T.fc1.w, T.fc1.ld, T.fc1.rows_pad, n_keep, D, (const int*)T.keep_dev, (const int*)nullptr);
  hipLaunchKernelGGL(gather_vector_kernel, dim3((T.fc1.rows_pad + 255) / 256), dim3(256), 0, dst->stream, S.fc1.b, T.fc1.b, T.fc1.rows_pad, n_keep, (const int*)T.keep_dev);
  hipLaunchKernelGGL(gather_matrix_kernel, dim3(2048), dim3(256), 0, dst->stream, S.fc2.w, S.fc2.ld, T.fc2.w, T.fc2.ld, T.fc2.rows_pad, D, n_keep, (const int*)nullptr, (const int*)T.keep_dev);
  HIPCHK(hipGetLastError());
  T.fc1.w_set = T.fc1.b_set = T.fc2.w_set = true;
  return 0;
}

int ssp2_act_l2_accum(void* stream, const void* act, int dtype, int n, int tokens, int d, int ld, int chain, int group,
                      float* norms_ws, float* out, size_t out_stride) {
  return act_l2_impl(stream, act, dtype, n, RowMap{tokens, 0, 0}, d, ld, chain, group, norms_ws, out, out_stride);
}

int ssp2_score_finish(void* hip_stream, const float* slab_dev, int n, int tokens, int group, int ld, int chain, float* norms_ws_dev,
                      float* out_dev, size_t out_stride) {
  if (!slab_dev || !norms_ws_dev || !out_dev) return fail(SSP2_EINVAL, "score_finish: null device pointer");
  if (n <= 0 || group < 0) return fail(SSP2_EINVAL, "score_finish: n=%d group=%d", n, group);
  if (tokens < GEMM_BM) return fail(SSP2_EINVAL, "score_finish: tokens=%d (the fused hook needs >= %d: a 128-row tile spans at most two samples)", tokens, GEMM_BM);
  if (ld < 1) return fail(SSP2_EINVAL, "score_finish: ld=%d", ld);
  if (out_stride < (size_t)ld) return fail(SSP2_EINVAL, "score_finish: out_stride=%zu < ld=%d", out_stride, ld);
  if (chain != SSP2_CHAIN_FP32 && chain != SSP2_CHAIN_BF16_REF) return fail(SSP2_EINVAL, "score_finish: chain=%d", chain);
  const RowMap rm = make_rowmap(tokens, n, group);
  if (total_rows(rm, n) > 0x7fffffffL) return fail(SSP2_EINVAL, "score_finish: too many rows");
  const int grp = (group <= 0 || group > n) ? n : group;
  return score_finish_fused((hipStream_t)hip_stream, slab_dev, n, rm, grp, ld, chain, norms_ws_dev, out_dev, out_stride);
}

int ssp2_peek_tensor(ssp2_handle e, int kind, int layer, int image, void* host, size_t bytes) {
  if (!e || !host) return fail(SSP2_EINVAL, "peek_tensor: null argument");
  IngestTarget t;
  if (int rc = resolve_tensor(e, kind, layer, &t)) return rc;
  const Mat* m = t.m;
  const void* src = nullptr;
  size_t want = 0;
  int32_t shape[5];
  switch (image) {
    case SSP2_PEEK_SHAPE:
      if (t.type == 0) { shape[0] = m->rows; shape[1] = m->cols; shape[2] = m->rows_pad; shape[3] = m->ld; shape[4] = m->w8 ? m->ld8 : 0; }
      else if (t.type == 1) { shape[0] = m->rows; shape[1] = 1; shape[2] = m->rows_pad; shape[3] = 1; shape[4] = 0; }
      else { shape[0] = shape[2] = (int32_t)t.expect; shape[1] = shape[3] = 1; shape[4] = 0; }
      if (bytes != sizeof shape) return fail(SSP2_EINVAL, "peek_tensor: the shape is %zu bytes, got %zu", sizeof shape, bytes);
      memcpy(host, shape, sizeof shape);
      return 0;
    case SSP2_PEEK_IMAGE:
      if (t.type == 0) { src = m->w; want = (size_t)m->rows_pad * m->ld * 2; }
      else if (t.type == 1) { src = m->b; want = (size_t)m->rows_pad * 4; }
      else { src = t.dst; want = t.expect * 4; }
      break;
    case SSP2_PEEK_E4M3:
    case SSP2_PEEK_SCALE:
      if (t.type != 0) return fail(SSP2_EINVAL, "peek_tensor: kind %d is no matrix: it has no e4m3 image", kind);
      if (!m->w8 || !m->wscale) return fail(SSP2_ESTATE, "peek_tensor: kind %d, layer %d has no e4m3 image (ssp2_set_precision quantises QKV, proj, fc1 and fc2)", kind, layer);
      if (image == SSP2_PEEK_E4M3) { src = m->w8; want = (size_t)m->rows_pad * m->ld8; }
      else { src = m->wscale; want = (size_t)m->rows_pad * 4; }
      break;
    default: return fail(SSP2_EINVAL, "peek_tensor: unknown image %d", image);
  }
  if (bytes != want) return fail(SSP2_EINVAL, "peek_tensor: kind %d, layer %d, image %d is %zu bytes, got %zu", kind, layer, image, want, bytes);
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(host, src, want, hipMemcpyDeviceToHost));
  return 0;
}

// The engine of an operator entry (ssp2_linear_*, ssp2_attention_*, ssp2_layernorm): a stack object that owns nothing, on the caller's
// stream and the current device, with the FORWARD'S DEFAULTS for the options a GEMM or LayerNorm launch reads — so that an entry is the
// forward's launch and not a copy of it.  rev >= 0: zigzag on, and next_dir() hands the entry's launch that direction (the forward
// alternates it); rev < 0: the forward walk.  Asks the device for its CU count (once): the entries call it after their argument checks.
static ssp2_engine op_engine(void* hip_stream, int rev = -1) {
  static int n_cu = 0;
  if (!n_cu) {
    int dev = 0; hipDeviceProp_t pr;
    n_cu = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256;
  }
  ssp2_engine e;
  e.stream = (hipStream_t)hip_stream; e.n_cu = n_cu; e.dev = cur_device();
  e.opt[SSP2_OPT_BIG_TILES] = e.opt[SSP2_OPT_FC1_BIG_TILES] = 1;
  e.opt[SSP2_OPT_BIG_TILE_MIN_ROWS] = kBigTileMinRowsDefault;
  { const char* v = getenv("SSP2_NT_STORES"); e.opt[SSP2_OPT_NT_STORES] = (v && *v) ? atoi(v) : 1; }      // the forward's default store policy
  if (rev >= 0) { e.opt[SSP2_OPT_ZIGZAG] = 1; e.zig = rev; }
  return e;
}
// ... of an attention entry: the geometry, and the forward's attention buffers pointed at the caller's
static ssp2_engine op_attn_engine(void* hip_stream, int rev, int tokens, int heads, int d_h, const uint16_t* qkv_dev, const uint16_t* q_dev, uint16_t* out_dev, int ldo) {
  ssp2_engine e = op_engine(hip_stream, rev);
  e.d.dim = heads * d_h; e.d.heads = heads; e.tokens = tokens; e.dh = d_h;
  e.qkvbuf = (bf16*)qkv_dev; e.q_cls = (bf16*)q_dev;
  e.obuf = e.o_cls = (bf16*)out_dev; e.o_ld = ldo;
  return e;
}
// what the three attention entries check alike: the counts, dim = heads * d_h, the bf16 output's row stride, the item count
static int check_attn_args(const char* who, int n, int tokens, int heads, int d_h, int group, const uint16_t* out_dev, int ldo) {
  if (n <= 0 || heads <= 0 || tokens <= 0 || group < 0) return fail(SSP2_EINVAL, "%s: n=%d heads=%d tokens=%d group=%d", who, n, heads, tokens, group);
  if ((long)heads * d_h > (1 << 20) || (heads * d_h) % 8) return fail(SSP2_EINVAL, "%s: dim = heads * d_h = %ld (a multiple of 8)", who, (long)heads * d_h);
  if (out_dev && (ldo < heads * d_h || ldo % 8)) return fail(SSP2_EINVAL, "%s: ldo=%d (>= dim %d, a multiple of 8)", who, ldo, heads * d_h);
  if ((long)n * heads > 0x7fffffffL) return fail(SSP2_EINVAL, "%s: too many attention items", who);
  return 0;
}
// what the two projection entries check of the epilogue's output: out / ldo (a multiple of ldo_mult) or x / ldx
static int check_linear_out(const char* who, int epilogue, const void* out_dev, int ldo, int ldo_mult, const float* x_dev, int ldx, int N) {
  if (epilogue == SSP2_EPI_BF16 || epilogue == SSP2_EPI_GELU) return (!out_dev || ldo < N || ldo % ldo_mult) ? fail(SSP2_EINVAL, "%s: out / ldo (>= N, a multiple of %d)", who, ldo_mult) : 0;
  if (epilogue == SSP2_EPI_RESID) return (!x_dev || ldx < N || ldx % 4) ? fail(SSP2_EINVAL, "%s: x / ldx", who) : 0;
  return fail(SSP2_EINVAL, "unknown epilogue %d", epilogue);
}

// The projection operator on its own (a3's building block): out = epilogue(A x W^T + bias) on caller-owned device
// buffers, routed to the same two kernels as the forward (persistent 256 x 256 tiles for M >= 4096 rows, 128 x 128
// otherwise; `kernel` = 1 / 2 forces the small / the large one — both give the same bits).
int ssp2_linear_bf16(void* hip_stream, int epilogue, const uint16_t* a_dev, int lda, const uint16_t* w_dev, int ldw, const float* bias_dev,
                     int M, int N, int K, uint16_t* out_dev, int ldo, float* x_dev, int ldx, int kernel) {
  if (!a_dev || !w_dev || !bias_dev) return fail(SSP2_EINVAL, "null operand");
  if (M <= 0 || N <= 0 || K <= 0 || (K % GEMM_BK) || (N % 64)) return fail(SSP2_EINVAL, "linear: M=%d N=%d K=%d (K multiple of %d, N multiple of 64)", M, N, K, GEMM_BK);
  if (lda < K || ldw < K || (lda % 8) || (ldw % 8)) return fail(SSP2_EINVAL, "linear: lda=%d ldw=%d must be >= K and multiples of 8", lda, ldw);
  if (kernel < 0 || kernel > 2) return fail(SSP2_EINVAL, "kernel selector %d", kernel);
  if (int rc = check_linear_out("linear", epilogue, out_dev, ldo, 8, x_dev, ldx, N)) return rc;
  ssp2_engine e = op_engine(hip_stream);
  // the kernel selector, said in the options the forward's routing (launch_gemm) reads: 1 = no big tiles, 2 = big tiles from the first row on
  if (kernel == 1) e.opt[SSP2_OPT_BIG_TILES] = 0;
  if (kernel == 2) e.opt[SSP2_OPT_BIG_TILE_MIN_ROWS] = 1;
  GemmArgs g = gemm_operands(act_bf16((const bf16*)a_dev, lda), w_dev, ldw, nullptr, bias_dev, M, N, K, ceil_to(N, 256) / GEMM_BN);
  g.out = (bf16*)out_dev; g.ldo = ldo; g.x = x_dev; g.ldx = ldx;
#ifdef SSP2_LAB
  if (epilogue == SSP2_EPI_RESID && e.opt[SSP2_OPT_BIG_TILES] && M >= big_tile_min_rows(&e) && N % 256 == 0 && K / 64 >= 4) {
    const char* v = getenv("SSP2_DEFER_RESID");     // SSP2_DEFER_RESID=1: the deferred residual, as the forward would take it
    if (v && atoi(v)) {
      static unsigned int* park[kMaxDevices] = {};
      if (!park[e.dev] && hipMalloc((void**)&park[e.dev], (size_t)e.n_cu * 131072) != hipSuccess) return fail(SSP2_ENOMEM, "linear: parking area");
      e.dg_scratch = park[e.dev]; e.opt[SSP2_OPT_DEFER_RESID] = 1;
    }
  }
#endif
  return dispatch_gemm(&e, epilogue, false, g, -2);
}

// ... with everything the forward's bf16 launches set besides: the residual read from xin, fc1's pre-GELU copy (out2: the unfused hook's
// operand, 128 x 128 kernel only) and its score sites, the walk direction.  The same dispatch_gemm(f8 = false) forms, no further one.
// Every argument is checked before the device is touched.
int ssp2_linear_bf16_ex(void* hip_stream, int epilogue, const uint16_t* a_dev, int lda, const uint16_t* w_dev, int ldw, const float* bias_dev,
                        int M, int N, int K, uint16_t* out_dev, int ldo, uint16_t* out2_dev, float* x_dev, const float* xin_dev, int ldx,
                        int score_site, int tokens, int group, int n_img, float* slab_dev, int slab_ld, int kernel, int rev) {
  if (!a_dev || !w_dev || !bias_dev) return fail(SSP2_EINVAL, "linear_ex: null operand");
  if (M <= 0 || N <= 0 || K <= 0 || (K % GEMM_BK) || (N % 64)) return fail(SSP2_EINVAL, "linear_ex: M=%d N=%d K=%d (K multiple of %d, N multiple of 64)", M, N, K, GEMM_BK);
  if (lda < K || ldw < K || (lda % 8) || (ldw % 8)) return fail(SSP2_EINVAL, "linear_ex: lda=%d ldw=%d must be >= K and multiples of 8", lda, ldw);
  if (kernel < 0 || kernel > 2) return fail(SSP2_EINVAL, "linear_ex: kernel selector %d", kernel);
  if (rev < 0 || rev > 1) return fail(SSP2_EINVAL, "linear_ex: rev=%d", rev);
  if (xin_dev && epilogue != SSP2_EPI_RESID) return fail(SSP2_EINVAL, "linear_ex: xin goes with the residual epilogue only");
  if (out2_dev && epilogue != SSP2_EPI_GELU) return fail(SSP2_EINVAL, "linear_ex: out2 (the pre-GELU copy) goes with the GELU epilogue only");
  if (out2_dev && kernel == 2) return fail(SSP2_EINVAL, "linear_ex: out2 is a form of the 128 x 128 kernel (kernel=2 refused)");
  if (score_site < 0 || score_site > 2 || (score_site && epilogue != SSP2_EPI_GELU)) return fail(SSP2_EINVAL, "linear_ex: score_site=%d (1 / 2 with the GELU epilogue only)", score_site);
  if (score_site) {
    if (tokens < GEMM_BM) return fail(SSP2_EINVAL, "linear_ex: the scoring epilogue needs tokens >= %d (tokens=%d)", GEMM_BM, tokens);
    if (!slab_dev || slab_ld <= 0 || slab_ld > N) return fail(SSP2_EINVAL, "linear_ex: slab / slab_ld=%d (1..N)", slab_ld);
    if (group < 0 || n_img <= 0) return fail(SSP2_EINVAL, "linear_ex: group=%d n_img=%d", group, n_img);
    if (total_rows(make_rowmap(tokens, n_img, group), n_img) > M)
      return fail(SSP2_EINVAL, "linear_ex: %d images of %d tokens in groups of %d exceed M=%d rows", n_img, tokens, group, M);
  }
  if (int rc = check_linear_out("linear_ex", epilogue, out_dev, ldo, 8, x_dev, ldx, N)) return rc;
  ssp2_engine e = op_engine(hip_stream, rev);
  if (kernel == 1) e.opt[SSP2_OPT_BIG_TILES] = 0;
  if (kernel == 2) e.opt[SSP2_OPT_BIG_TILE_MIN_ROWS] = 1;
  GemmArgs g = gemm_operands(act_bf16((const bf16*)a_dev, lda), w_dev, ldw, nullptr, bias_dev, M, N, K, ceil_to(N, 256) / GEMM_BN);
  g.out = (bf16*)out_dev; g.out2 = (bf16*)out2_dev; g.ldo = ldo; g.x = x_dev; g.xin = xin_dev; g.ldx = ldx;
  if (score_site) {
    const RowMap rm = make_rowmap(tokens, n_img, group);
    g.score_site = score_site; g.tokens = tokens; g.slab = slab_dev; g.slab_ld = slab_ld; g.n_img = n_img; g.group = rm.group; g.mpad = rm.mpad;
    // the slab has an entry per 128 rows of ceil256(M): the 256 x 256 kernel writes both entries of its last tile, the 128 x 128 kernel
    // has no tile for an odd last one — it is zeroed here, so that both leave the same slab
    const int t128 = (M + GEMM_BM - 1) / GEMM_BM;
    if (t128 & 1) HIPCHK(hipMemsetAsync(slab_dev + (size_t)t128 * 2 * slab_ld, 0, (size_t)2 * slab_ld * sizeof(float), e.stream));
  }
  return dispatch_gemm(&e, epilogue, false, g, -2);
}

// The fp8 projection operator on its own: the forward's launch_gemm256<EPI, SCORE, true> (QKV, fc1 with its score sites, the
// residual projections) on caller-owned e4m3 operands.  Every argument is checked before the device is touched.
int ssp2_linear_e4m3(void* hip_stream, int epilogue, const uint8_t* a_dev, int lda, const float* ascale_dev, float ascale_const,
                     const uint8_t* w_dev, int ldw, const float* wscale_dev, const float* bias_dev, int M, int N, int K,
                     void* out_dev, int ldo, float* x_dev, const float* xin_dev, int ldx,
                     int score_site, int tokens, int group, int n_img, float* slab_dev, int slab_ld, int rev) {
  if (!a_dev || !w_dev || !bias_dev) return fail(SSP2_EINVAL, "linear_e4m3: null operand");
  if (rev < 0 || rev > 1) return fail(SSP2_EINVAL, "linear_e4m3: rev=%d", rev);
  if (!wscale_dev) return fail(SSP2_EINVAL, "linear_e4m3: the weight rows' scales (wscale) are required");
  if (M <= 0 || N <= 0 || K <= 0 || (K % 128) || (N % 64)) return fail(SSP2_EINVAL, "linear_e4m3: M=%d N=%d K=%d (K multiple of 128, N multiple of 64)", M, N, K);
  if (lda < K || ldw < K || (lda % 16) || (ldw % 16)) return fail(SSP2_EINVAL, "linear_e4m3: lda=%d ldw=%d must be >= K and multiples of 16", lda, ldw);
  if (!std::isfinite(ascale_const) || ascale_const < 0.f) return fail(SSP2_EINVAL, "linear_e4m3: ascale_const=%g", ascale_const);
  if (ascale_dev && ascale_const != 0.f) return fail(SSP2_EINVAL, "linear_e4m3: per-row ascale and ascale_const are exclusive");
  if (score_site < 0 || score_site > 2 || (score_site && epilogue != SSP2_EPI_GELU)) return fail(SSP2_EINVAL, "linear_e4m3: score_site=%d (1 / 2 with the GELU epilogue only)", score_site);
  if (score_site) {
    if (tokens < GEMM_BM) return fail(SSP2_EINVAL, "linear_e4m3: the scoring epilogue needs tokens >= %d (tokens=%d)", GEMM_BM, tokens);
    if (!slab_dev || slab_ld <= 0 || slab_ld > N) return fail(SSP2_EINVAL, "linear_e4m3: slab / slab_ld=%d (1..N)", slab_ld);
    if (group < 0 || n_img <= 0) return fail(SSP2_EINVAL, "linear_e4m3: group=%d n_img=%d", group, n_img);
    if (total_rows(make_rowmap(tokens, n_img, group), n_img) > M)
      return fail(SSP2_EINVAL, "linear_e4m3: %d images of %d tokens in groups of %d exceed M=%d rows", n_img, tokens, group, M);
  }
  if (int rc = check_linear_out("linear_e4m3", epilogue, out_dev, ldo, epilogue == SSP2_EPI_GELU ? 16 : 8, x_dev, ldx, N)) return rc;      // (GELU: e4m3 bytes out, ldo in bytes)
  ssp2_engine e = op_engine(hip_stream, rev);
  GemmArgs g = gemm_operands(act_e4m3(a_dev, lda, ascale_dev, ascale_const), w_dev, ldw, wscale_dev, bias_dev, M, N, K, 0);
  g.out = (bf16*)out_dev; g.ldo = ldo; g.x = x_dev; g.xin = xin_dev; g.ldx = ldx;
  if (score_site) {
    const RowMap rm = make_rowmap(tokens, n_img, group);
    g.score_site = score_site; g.tokens = tokens; g.slab = slab_dev; g.slab_ld = slab_ld; g.n_img = n_img; g.group = rm.group; g.mpad = rm.mpad;
  }
  return dispatch_gemm(&e, epilogue, true, g, -2);
}

// The residual projections with LayerScale on their own (EPI_RESID_LS): the launches of ssp2_linear_bf16 / ssp2_linear_e4m3 with the
// residual epilogue, plus the branch's fp32 scale.  Every argument is checked before the device is touched.
int ssp2_linear_ls_bf16(void* hip_stream, const uint16_t* a_dev, int lda, const uint16_t* w_dev, int ldw, const float* bias_dev,
                        const float* gamma_dev, int M, int N, int K, float* x_dev, const float* xin_dev, int ldx, int kernel, int rev) {
  if (!a_dev || !w_dev || !bias_dev) return fail(SSP2_EINVAL, "linear_ls: null operand");
  if (!gamma_dev) return fail(SSP2_EINVAL, "linear_ls: null gamma");
  if ((uintptr_t)gamma_dev & 15) return fail(SSP2_EINVAL, "linear_ls: gamma must be 16-byte aligned (the epilogues read it four columns at a time)");
  if (M <= 0 || N <= 0 || K <= 0 || (K % GEMM_BK) || (N % 64)) return fail(SSP2_EINVAL, "linear_ls: M=%d N=%d K=%d (K multiple of %d, N multiple of 64)", M, N, K, GEMM_BK);
  if (lda < K || ldw < K || (lda % 8) || (ldw % 8)) return fail(SSP2_EINVAL, "linear_ls: lda=%d ldw=%d must be >= K and multiples of 8", lda, ldw);
  if (kernel < 0 || kernel > 2) return fail(SSP2_EINVAL, "linear_ls: kernel selector %d", kernel);
  if (rev < 0 || rev > 1) return fail(SSP2_EINVAL, "linear_ls: rev=%d", rev);
  if (int rc = check_linear_out("linear_ls", SSP2_EPI_RESID, nullptr, 0, 8, x_dev, ldx, N)) return rc;
  ssp2_engine e = op_engine(hip_stream, rev);
  if (kernel == 1) e.opt[SSP2_OPT_BIG_TILES] = 0;
  if (kernel == 2) e.opt[SSP2_OPT_BIG_TILE_MIN_ROWS] = 1;
  GemmArgs g = gemm_operands(act_bf16((const bf16*)a_dev, lda), w_dev, ldw, nullptr, bias_dev, M, N, K, ceil_to(N, 256) / GEMM_BN);
  g.x = x_dev; g.xin = xin_dev; g.ldx = ldx; g.ls = gamma_dev;
  return dispatch_gemm(&e, EPI_RESID_LS, false, g, -2);
}
int ssp2_linear_ls_e4m3(void* hip_stream, const uint8_t* a_dev, int lda, const float* ascale_dev, float ascale_const, const uint8_t* w_dev, int ldw,
                        const float* wscale_dev, const float* bias_dev, const float* gamma_dev, int M, int N, int K, float* x_dev,
                        const float* xin_dev, int ldx, int rev) {
  if (!a_dev || !w_dev || !bias_dev) return fail(SSP2_EINVAL, "linear_ls_e4m3: null operand");
  if (!gamma_dev) return fail(SSP2_EINVAL, "linear_ls_e4m3: null gamma");
  if ((uintptr_t)gamma_dev & 15) return fail(SSP2_EINVAL, "linear_ls_e4m3: gamma must be 16-byte aligned (the epilogues read it four columns at a time)");
  if (rev < 0 || rev > 1) return fail(SSP2_EINVAL, "linear_ls_e4m3: rev=%d", rev);
  if (!wscale_dev) return fail(SSP2_EINVAL, "linear_ls_e4m3: the weight rows' scales (wscale) are required");
  if (M <= 0 || N <= 0 || K <= 0 || (K % 128) || (N % 64)) return fail(SSP2_EINVAL, "linear_ls_e4m3: M=%d N=%d K=%d (K multiple of 128, N multiple of 64)", M, N, K);
  if (lda < K || ldw < K || (lda % 16) || (ldw % 16)) return fail(SSP2_EINVAL, "linear_ls_e4m3: lda=%d ldw=%d must be >= K and multiples of 16", lda, ldw);
  if (!std::isfinite(ascale_const) || ascale_const < 0.f) return fail(SSP2_EINVAL, "linear_ls_e4m3: ascale_const=%g", ascale_const);
  if (ascale_dev && ascale_const != 0.f) return fail(SSP2_EINVAL, "linear_ls_e4m3: per-row ascale and ascale_const are exclusive");
  if (int rc = check_linear_out("linear_ls_e4m3", SSP2_EPI_RESID, nullptr, 0, 8, x_dev, ldx, N)) return rc;
  ssp2_engine e = op_engine(hip_stream, rev);
  GemmArgs g = gemm_operands(act_e4m3(a_dev, lda, ascale_dev, ascale_const), w_dev, ldw, wscale_dev, bias_dev, M, N, K, 0);
  g.x = x_dev; g.xin = xin_dev; g.ldx = ldx; g.ls = gamma_dev;
  return dispatch_gemm(&e, EPI_RESID_LS, true, g, -2);
}

// The weight quantiser on its own: what quantise_mat launches (quant_rows_e4m3_kernel), on caller-owned buffers.
int ssp2_quantise_rows_e4m3(void* hip_stream, const uint16_t* w_dev, int ld, int rows, int cols, int rows_pad, uint8_t* w8_dev, int ld8, float* scale_dev) {
  if (!w_dev || !w8_dev || !scale_dev) return fail(SSP2_EINVAL, "quantise_rows_e4m3: null buffer");
  if (rows <= 0 || cols <= 0 || ld < cols || rows_pad < rows) return fail(SSP2_EINVAL, "quantise_rows_e4m3: rows=%d cols=%d ld=%d rows_pad=%d", rows, cols, ld, rows_pad);
  if (ld8 < cols || ld8 % 16) return fail(SSP2_EINVAL, "quantise_rows_e4m3: ld8=%d (>= cols %d, a multiple of 16)", ld8, cols);
  hipLaunchKernelGGL(quant_rows_e4m3_kernel, dim3((rows_pad + 3) / 4), dim3(256), 0, (hipStream_t)hip_stream, (const bf16*)w_dev, ld, w8_dev, ld8, scale_dev, rows, cols, rows_pad);
  HIPCHK(hipGetLastError());
  return 0;
}

// Multi-head attention on its own, on caller-owned buffers: a temporary engine with the forward's buffers pointed at the caller's,
// then launch_attn — the routing and the instantiations of the forward (persistent / one-item kernel, LIVE, CLS-only tail).  Every
// argument is checked before the device is touched.
int ssp2_attention_bf16(void* hip_stream, const uint16_t* qkv_dev, int n, int tokens, int heads, int d_h, int group,
                        const uint16_t* q_cls_dev, uint16_t* out_dev, int ldo, uint8_t* out8_dev, int ldo8, float out8_scale,
                        unsigned int* sat_dev, int persist, int live, int rev) {
  if (!qkv_dev) return fail(SSP2_EINVAL, "attention: null qkv");
  if (int rc = check_attn_args("attention", n, tokens, heads, d_h, group, out_dev, ldo)) return rc;
  if (!attn_supported(d_h, tokens)) return fail(SSP2_EINVAL, "attention kernel not instantiated for d_h=%d, tokens=%d", d_h, tokens);
  const int dim = heads * d_h;
  if (persist < -1 || persist > 1 || live < -1 || live > 1 || rev < 0 || rev > 1) return fail(SSP2_EINVAL, "attention: persist=%d live=%d rev=%d", persist, live, rev);
  if (!out_dev && !out8_dev) return fail(SSP2_EINVAL, "attention: no output");
  if (q_cls_dev && (out8_dev || !out_dev)) return fail(SSP2_EINVAL, "attention: the CLS-only form writes bf16 only");
  if (out8_dev && (ldo8 < dim || ldo8 % 16 || !(out8_scale > 0.f) || out8_scale > 65536.f)) return fail(SSP2_EINVAL, "attention: ldo8=%d out8_scale=%g", ldo8, out8_scale);
  if (out8_dev && !attn_persistent_for(0, persist < 0 ? 1 : persist, d_h, tokens))
    return fail(SSP2_EINVAL, "attention: the e4m3 output needs a persistent kernel (d_h = 64 with 97..224 tokens, d_h = 80 with 257)");
  ssp2_engine e = op_attn_engine(hip_stream, rev, tokens, heads, d_h, qkv_dev, q_cls_dev, out_dev, out_dev ? ldo : dim);      // (rev: the persistent kernels' walk)
  e.opt[SSP2_OPT_ATTN_PERSIST] = persist < 0 ? 1 : persist;
  e.opt[SSP2_OPT_ATTN_LIVE] = live < 0 ? 1 : live;
  e.ld8_dim = ldo8; e.fp8_sat = sat_dev;
  return launch_attn(&e, n, make_rowmap(tokens, n, group), q_cls_dev != nullptr, out8_dev, out8_scale);
}

// The key-streaming attention on its own (attn_stream.hip.h), on caller-owned buffers; every argument checked before the device.
int ssp2_attention_stream_bf16(void* hip_stream, const uint16_t* qkv_dev, int n, int tokens, int heads, int d_h, int group,
                               const uint16_t* q_cls_dev, uint16_t* out_dev, int ldo) {
  if (!qkv_dev || !out_dev) return fail(SSP2_EINVAL, "attention_stream: null qkv / out");
  if (int rc = check_attn_args("attention_stream", n, tokens, heads, d_h, group, out_dev, ldo)) return rc;
  if (d_h != 64) return fail(SSP2_EINVAL, "attention_stream: d_h=%d (64 only)", d_h);
  if (tokens > ATTN_STREAM_MAX_TOKENS) return fail(SSP2_EINVAL, "attention_stream: tokens=%d (1..%d)", tokens, ATTN_STREAM_MAX_TOKENS);
  if ((long)n * heads * ((tokens + 32 * ATTN_STREAM_QW - 1) / (32 * ATTN_STREAM_QW)) > 0x7fffffffL) return fail(SSP2_EINVAL, "too many attention items");
  ssp2_engine e = op_attn_engine(hip_stream, -1, tokens, heads, d_h, qkv_dev, q_cls_dev, out_dev, ldo);
  e.opt[SSP2_OPT_ATTN_STREAM] = 2;
  return launch_attn_stream(&e, n, make_rowmap(tokens, n, group), q_cls_dev != nullptr);
}

// ... its OUT8 form (attn64_stream_kernel<true>): e4m3(o * out8_scale) bytes, the clipping waves counted into *sat_dev (may be null)
int ssp2_attention_stream_e4m3(void* hip_stream, const uint16_t* qkv_dev, int n, int tokens, int heads, int d_h, int group,
                               uint8_t* out8_dev, int ldo8, float out8_scale, unsigned int* sat_dev) {
  if (!qkv_dev || !out8_dev) return fail(SSP2_EINVAL, "attention_stream_e4m3: null qkv / out8");
  if (int rc = check_attn_args("attention_stream_e4m3", n, tokens, heads, d_h, group, nullptr, 0)) return rc;
  if (d_h != 64) return fail(SSP2_EINVAL, "attention_stream_e4m3: d_h=%d (64 only)", d_h);
  if (tokens > ATTN_STREAM_MAX_TOKENS) return fail(SSP2_EINVAL, "attention_stream_e4m3: tokens=%d (1..%d)", tokens, ATTN_STREAM_MAX_TOKENS);
  if ((long)n * heads * ((tokens + 32 * ATTN_STREAM_QW - 1) / (32 * ATTN_STREAM_QW)) > 0x7fffffffL) return fail(SSP2_EINVAL, "too many attention items");
  if (ldo8 < heads * 64 || ldo8 % 16 || ((uintptr_t)out8_dev & 15))
    return fail(SSP2_EINVAL, "attention_stream_e4m3: out8 / ldo8=%d (16-byte aligned, >= dim %d, a multiple of 16)", ldo8, heads * 64);
  int ex = 0;
  if (!(out8_scale > 0.f) || !std::isfinite(out8_scale) || frexpf(out8_scale, &ex) != 0.5f)
    return fail(SSP2_EINVAL, "attention_stream_e4m3: out8_scale must be a power of two > 0 (got %g)", out8_scale);
  ssp2_engine e = op_attn_engine(hip_stream, -1, tokens, heads, d_h, qkv_dev, nullptr, nullptr, heads * 64);
  e.opt[SSP2_OPT_ATTN_STREAM] = 2; e.opt[SSP2_OPT_STREAM_FP8] = 1;
  e.ld8_dim = ldo8; e.fp8_sat = sat_dev;
  return launch_attn_stream(&e, n, make_rowmap(tokens, n, group), false, out8_dev, out8_scale);
}

// The tail's prefix-query attention on its own (n_prefix queries per image, prefix-major q and out), on the resident CLS-only kernels or,
// stream != 0, the key-streaming one: a temporary engine whose tail carries n_prefix rows, then the forward's launch.
int ssp2_attention_prefix_bf16(void* hip_stream, const uint16_t* qkv_dev, int n, int tokens, int heads, int d_h, int group,
                               const uint16_t* q_dev, uint16_t* out_dev, int ldo, int n_prefix, int stream) {
  if (!qkv_dev || !q_dev || !out_dev) return fail(SSP2_EINVAL, "attention_prefix: null qkv / q / out");
  if (int rc = check_attn_args("attention_prefix", n, tokens, heads, d_h, group, out_dev, ldo)) return rc;
  if (n_prefix < 1 || n_prefix > 2) return fail(SSP2_EINVAL, "attention_prefix: n_prefix=%d (1 or 2)", n_prefix);
  if (n_prefix > tokens) return fail(SSP2_EINVAL, "attention_prefix: n_prefix=%d > tokens=%d", n_prefix, tokens);
  if (stream < 0 || stream > 1) return fail(SSP2_EINVAL, "attention_prefix: stream=%d (0 resident, 1 key-streaming)", stream);
  if (stream ? !attn_stream_ok(d_h, tokens) : !attn_resident(d_h, tokens))
    return fail(SSP2_EINVAL, "attention_prefix: no %s kernel for d_h=%d, tokens=%d", stream ? "key-streaming" : "resident", d_h, tokens);
  if ((long)n_prefix * n * ldo > 0x7fffffffL || (long)n * heads * d_h > 0x7fffffffL) return fail(SSP2_EINVAL, "attention_prefix: n=%d too large", n);
  ssp2_engine e = op_attn_engine(hip_stream, -1, tokens, heads, d_h, qkv_dev, q_dev, out_dev, ldo);
  e.tail_rows = n_prefix;
  e.opt[SSP2_OPT_ATTN_STREAM] = stream ? 2 : 0;
  return launch_attn(&e, n, make_rowmap(tokens, n, group), true);
}

// LayerNorm on its own, on caller-owned buffers: launch_ln of a temporary engine (the forward's MAXV / FULL dispatch and its
// reverse-walk rule: `rev` takes effect from kBigTileMinRowsDefault rows on, as in the forward).
int ssp2_layernorm(void* hip_stream, const float* x_dev, size_t in_stride, int rows, int D, const float* gamma_dev, const float* beta_dev,
                   float eps, int gather_tokens, int gather_group, uint16_t* y_dev, int out_ld, uint8_t* y8_dev, float* ascale_dev, int rev) {
  if (!x_dev || !gamma_dev || !beta_dev) return fail(SSP2_EINVAL, "layernorm: null operand");
  if (rows <= 0 || D <= 0 || D % 4 || D > 2048) return fail(SSP2_EINVAL, "layernorm: rows=%d D=%d (D a multiple of 4, <= 2048)", rows, D);
  if (!(eps >= 0.f) || !std::isfinite(eps)) return fail(SSP2_EINVAL, "layernorm: eps=%g", eps);
  if (gather_tokens < 0 || gather_group < 0 || rev < 0 || rev > 1) return fail(SSP2_EINVAL, "layernorm: gather_tokens=%d gather_group=%d rev=%d", gather_tokens, gather_group, rev);
  if (gather_tokens == 0 && (in_stride < (size_t)D || in_stride % 4)) return fail(SSP2_EINVAL, "layernorm: in_stride=%zu (>= D, a multiple of 4)", in_stride);
  if (!y_dev == !y8_dev) return fail(SSP2_EINVAL, "layernorm: exactly one of y (bf16) and y8 (e4m3) is written");
  if (y8_dev && !ascale_dev) return fail(SSP2_EINVAL, "layernorm: the e4m3 form writes per-row scales (ascale)");
  if (out_ld < D || out_ld % 4) return fail(SSP2_EINVAL, "layernorm: out_ld=%d (>= D, a multiple of 4)", out_ld);
  ssp2_engine e = op_engine(hip_stream, rev);
  e.d.ln_eps = eps;
  const RowMap gather = gather_tokens > 0 ? make_rowmap(gather_tokens, rows, gather_group) : RowMap{0, 0, 0};
  return launch_ln(&e, x_dev, in_stride, gamma_dev, beta_dev, (bf16*)y_dev, out_ld, rows, D, gather, y8_dev, y8_dev ? ascale_dev : nullptr);
}

int ssp2_profile_begin(ssp2_handle e, int klass) {
  if (!e || klass < 0 || klass > SSP2_K_COUNT) return fail(SSP2_EINVAL, "bad profile class");      // SSP2_K_COUNT = every class
  for (auto& pr : e->prof_events) { hipEventDestroy(pr.a); hipEventDestroy(pr.b); }
  e->prof_events.clear();
  for (int k = 0; k < SSP2_K_COUNT; ++k) e->prof_flops[k] = e->prof_bytes[k] = 0;
  e->prof_class = klass;
  return 0;
}

// per-class totals of the launches recorded since ssp2_profile_begin (synchronises the stream; leaves the recording on)
int ssp2_profile_query(ssp2_handle e, int klass, double* total_ms, int64_t* launches, double* flops, double* bytes) {
  if (!e || klass < 0 || klass >= SSP2_K_COUNT) return fail(SSP2_EINVAL, "bad profile class");
  HIPCHK(hipStreamSynchronize(e->stream));
  double tot = 0; int64_t cnt = 0;
  for (auto& pr : e->prof_events) {
    if (pr.klass != klass) continue;
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, pr.a, pr.b));
    tot += ms; ++cnt;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = cnt;
  if (flops) *flops = e->prof_flops[klass];
  if (bytes) *bytes = e->prof_bytes[klass];
  return 0;
}

int ssp2_profile_end(ssp2_handle e, double* total_ms, int64_t* launches, double* gemm_flops) {
  if (!e) return fail(SSP2_EINVAL, "null handle");
  HIPCHK(hipStreamSynchronize(e->stream));
  double tot = 0, fl = 0;
  for (auto& pr : e->prof_events) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, pr.a, pr.b));
    tot += ms;
    hipEventDestroy(pr.a); hipEventDestroy(pr.b);
  }
  for (int k = 0; k < SSP2_K_COUNT; ++k) fl += e->prof_flops[k];
  if (total_ms) *total_ms = tot;
  if (launches) *launches = (int64_t)e->prof_events.size();
  if (gemm_flops) *gemm_flops = fl;
  e->prof_events.clear();
  e->prof_class = -1;
  return 0;
}

// ------------------------------------------------------------------------------------------------ f4: input pipeline
struct ssp2_preproc {
  int in_h = 0, in_w = 0, out = 0, ks_h = 0, ks_v = 0;
  int *bounds_h = nullptr, *kk_h = nullptr, *bounds_v = nullptr, *kk_v = nullptr;
  float mean[3], sd[3];
};

static double bicubic_filter(double x) {                 // Pillow Resample.c, a = -0.5
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// Pillow precompute_coeffs + normalize_coeffs_8bpc for the full input range [0, in_size)
static int pil_coeffs(int in_size, int out_size, std::vector<int>& bounds, std::vector<int>& kk) {
  const double scale = (double)in_size / out_size;
  double filterscale = scale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = 2.0 * filterscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  bounds.assign((size_t)out_size * 2, 0);
  kk.assign((size_t)out_size * ksize, 0);
  std::vector<double> pre(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    double ww = 0.0;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    int x = 0;
    for (; x < xmax; ++x) { const double w = bicubic_filter((x + xmin - center + 0.5) * ss); pre[x] = w; ww += w; }
    for (x = 0; x < xmax; ++x) if (ww != 0.0) pre[x] /= ww;
    for (; x < ksize; ++x) pre[x] = 0;
    for (x = 0; x < ksize; ++x)
      kk[(size_t)xx * ksize + x] = pre[x] < 0 ? (int)(-0.5 + pre[x] * (1 << PREPROC_PRECISION_BITS)) : (int)(0.5 + pre[x] * (1 << PREPROC_PRECISION_BITS));
    bounds[2 * xx] = xmin; bounds[2 * xx + 1] = xmax;
  }
  return ksize;
}

int ssp2_preproc_create(int in_h, int in_w, int out_size, const float* mean3, const float* std3, ssp2_preproc_handle* out) {
  if (!out || !mean3 || !std3 || in_h <= 0 || in_w <= 0 || out_size <= 0) return fail(SSP2_EINVAL, "bad preproc arguments");
  auto* p = new ssp2_preproc();
  p->in_h = in_h; p->in_w = in_w; p->out = out_size;
  for (int i = 0; i < 3; ++i) { p->mean[i] = mean3[i]; p->sd[i] = std3[i]; }
  std::vector<int> bh, kh, bv, kv;
  p->ks_h = pil_coeffs(in_w, out_size, bh, kh);
  p->ks_v = pil_coeffs(in_h, out_size, bv, kv);
  auto up = [](int** d, const std::vector<int>& v) {
    if (hipMalloc((void**)d, v.size() * 4) != hipSuccess) return false;
    return hipMemcpy(*d, v.data(), v.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
  };
  if (!up(&p->bounds_h, bh) || !up(&p->kk_h, kh) || !up(&p->bounds_v, bv) || !up(&p->kk_v, kv)) { ssp2_preproc_destroy(p); return fail(SSP2_ENOMEM, "preproc tables"); }
  *out = p;
  return 0;
}

int ssp2_preproc_destroy(ssp2_preproc_handle p) {
  if (!p) return 0;
  hipFree(p->bounds_h); hipFree(p->kk_h); hipFree(p->bounds_v); hipFree(p->kk_v);
  delete p;
  return 0;
}

int ssp2_preproc_run(ssp2_preproc_handle p, void* stream, const uint8_t* img_dev, int n, const uint8_t* hflip_dev, uint8_t* tmp_dev,
                     float* out_dev, uint8_t* out_u8_dev) {
  if (!p || !img_dev || !tmp_dev || !out_dev || n <= 0) return fail(SSP2_EINVAL, "bad preproc_run arguments");
  hipStream_t s = (hipStream_t)stream;
  const long t1 = (long)n * p->in_h * p->out * 3, t2 = (long)n * 3 * p->out * p->out;
  hipLaunchKernelGGL(resize_h_u8_kernel, dim3((unsigned)std::min<long>((t1 + 255) / 256, 65536)), dim3(256), 0, s, img_dev, tmp_dev, n, p->in_h, p->in_w,
                     p->out, p->bounds_h, p->kk_h, p->ks_h);
  hipLaunchKernelGGL(resize_v_norm_kernel, dim3((unsigned)std::min<long>((t2 + 255) / 256, 65536)), dim3(256), 0, s, tmp_dev, out_dev, out_u8_dev, n, p->in_h,
                     p->out, p->out, p->bounds_v, p->kk_v, p->ks_v, hflip_dev, p->mean[0], p->mean[1], p->mean[2], p->sd[0], p->sd[1], p->sd[2]);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"

static int act_l2_impl(void* stream, const void* act, int dtype, int n, RowMap rm, int d, int ld, int chain, int group,
                       float* norms_ws, float* out, size_t out_stride) {
  const int tokens = rm.tokens;
  if (!act || !norms_ws || !out) return fail(SSP2_EINVAL, "null device pointer");
  if (n <= 0 || tokens <= 0 || d <= 0 || ld < d || (ld % 8)) return fail(SSP2_EINVAL, "bad shape n=%d tokens=%d d=%d ld=%d (ld multiple of 8, >= d)", n, tokens, d, ld);
  // every column j < ld of a group's row is written: a smaller stride would let one group's block write into the next group's row
  if (out_stride < (size_t)ld) return fail(SSP2_EINVAL, "out_stride=%zu < ld=%d", out_stride, ld);
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((ld + 511) / 512, n, 2), blk(256);       // z = token half (see act_l2_norms_kernel)
  // non-temporal loads: the activation is read once (5.28 -> 5.78 TB/s on the 512-image tensor, profiles/r02_d_act_l2_nt_ab.txt)
  if (dtype == 0)
    hipLaunchKernelGGL((act_l2_norms_kernel<bf16, 1>), grid, blk, 0, s, (const bf16*)act, norms_ws, rm, ld, n);
  else if (dtype == 1)
    hipLaunchKernelGGL((act_l2_norms_kernel<float, 1>), grid, blk, 0, s, (const float*)act, norms_ws, rm, ld, n);
  else
    return fail(SSP2_EINVAL, "dtype %d (0 = bf16, 1 = f32)", dtype);
  const int grp = (group <= 0 || group > n) ? n : group;
  hipLaunchKernelGGL(score_colsum_halves_kernel, dim3((ld + 63) / 64, (n + grp - 1) / grp), dim3(256), 0, s, norms_ws, out, out_stride, n, grp, ld,
                     chain);
  HIPCHK(hipGetLastError());
  return 0;
}

