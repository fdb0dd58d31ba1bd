// Large-tile bf16 MFMA GEMM for the big-M projections (QKV, attention out-proj, fc1 of evaluation passes, fc2):
// 256 x 256 x 64 tiles, 8 waves (2 along M x 4 along N, 128 x 64 per wave), ONE persistent workgroup per CU that
// walks tiles wg, wg+G, wg+2G, ...  Results are bit-identical to gemm_bf16_kernel (same K order, same rounding
// points); csrc/tools/gemm_bench.hip checks that on every run.
//
// LDS (all 160 KiB, one array):   A0 | A1 | B0 | B1 | A2     32 KiB each
//   main loop   asymmetric ring as in gemm.hip.h: the A panel (streams from HBM / Infinity Cache) is three K-tiles
//               deep, the weight panel (L2-resident) two, filled by 16-byte LDS-DMA (1-KiB pieces, 8 per wave per
//               K-tile).  The two wave groups (waves 0-3 / 4-7 = the two waves of every SIMD) run in PING-PONG,
//               half a K-tile per step: one group reads its 12 fragments from LDS while the other issues 16 MFMAs
//               with its 4 DMA pieces between them (see the phase table at the loop); 4 raw s_barriers and ONE
//               counted `s_waitcnt vmcnt(4)` per K-tile, so A(kt+2) stays in flight across the K-tile boundary.
//               The steady-state K-tile body is a separate compile-time instance without any conditional.
//   tile change right after the last K-tile the NEXT tile's B(0), A(0), A(1) go out into B0, A0, A1; the epilogue
//               then runs out of B1 | A2 (64 KiB = 8 KiB per wave, wave-private, no barrier inside).  vmcnt counts
//               loads, stores and LDS-DMA together in issue order, so the next main loop starts behind a counted
//               wait that leaves only the epilogue's LAST stores in flight — nothing is ever drained to zero between
//               two main loops (full tiles; an edge tile takes the conservative vmcnt(0) path).
//
// Epilogues: the MFMA operands are swapped (acc = W_frag x A_frag), so a lane owns ONE output row and FOUR
// consecutive columns per register quad.  Against the row-of-4-rows layout of the plain order this makes the bias
// add and the bf16 conversion packed and replaces 16 two-byte LDS stores per 32x32 block by 4 eight-byte ones;
// outputs leave through a wave-private LDS tile as whole 128-byte row segments.  The residual epilogue keeps 16
// coalesced loads of the fp32 x tile in flight per wave (raw-buffer addressing: no 64-bit address registers) and
// adds the accumulators to them in that row-contiguous layout.  The stage-1 scoring variant keeps the plain operand
// order (see the template comment).
#pragma once
#include "gemm.hip.h"
#include <type_traits>
#ifndef STAMP
#define STAMP(slot) do {} while (0)
#endif
#ifdef GEMM_STAMPS
#define TSTAMP(slot) do { if (tiles_done == 3) STAMP(slot); } while (0)
#define RSTAMP(slot) do { if (tid == 0) { unsigned long long t_; asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); g.stamps[(size_t)blockIdx.x * 64 + (slot)] = t_; } } while (0)
#else
#define TSTAMP(slot) do {} while (0)
#define RSTAMP(slot) do {} while (0)
#endif

// Cache policy of the streamed traffic (activation panel, x tile, outputs).  GEMM_NT = 1 marks all of it non-temporal
// so that it cannot evict the weight panels from the XCD's 4 MiB L2; 2 = the LDS-DMA loads only, 3 = the stores only.
// Measured (gemm_bench + rocprofv3 PMC, 63040-row shapes, interleaved runs): with NT loads QKV's HBM-side fetch halves
// (182 -> 99 MB per launch, L2 hit rate 72 -> 79 %) and yet every shape runs 5-9 % SLOWER; NT stores alone are within
// noise of the default.  The default policy stays; the switch is kept for A/B runs only.
// LDS-DMA pieces (of 4 per unit) issued in the LOAD phase instead of between the MFMAs.  Measured on the 63040-row
// shapes (interleaved runs): 1 -> 1-2 % slower, 2 -> 3 % slower, 4 (a burst, ~140 cycles per piece) -> 25 % slower than
// 0, although the loading wave then idles ~400 cycles per phase at the barrier: a piece issued beside the partner's
// MFMAs slows those down by more than it saves.  Kept as a switch for A/B runs.
#ifndef PP_NL
#define PP_NL 0
#endif
#ifndef GEMM_NT
#define GEMM_NT 0
#endif
#ifndef GEMM_MFMA16
#define GEMM_MFMA16 0
#endif
#if GEMM_NT == 2
#define GLDS_A glds16_nt
#define ST_OUT(p, v) (*(p) = (v))
#elif GEMM_NT == 3
#define GLDS_A glds16
#define ST_OUT(p, v) __builtin_nontemporal_store((v), (p))
#elif GEMM_NT
#define GLDS_A glds16_nt
#define ST_OUT(p, v) __builtin_nontemporal_store((v), (p))
#else
#define GLDS_A glds16
#ifdef GEMM_ABL_NOSTORE   // ablation (timing builds of tools/gemm_bench only): the bf16 / GELU epilogue keeps its arithmetic and
#define ST_OUT(p, v) asm volatile("" :: "v"(v))   // its LDS round trip but sends nothing to memory
#else
#define ST_OUT(p, v) (*(p) = (v))
#endif
#endif

struct G256 {
  static constexpr int BM = 256, BN = 256, NW = 8;
  static constexpr int TM = 4, TN = 2;                  // 32x32 MFMA tiles per wave along M / N
  static constexpr int SLOT = 32768;                    // 256 rows x 64 bf16
  static constexpr int A0 = 0, A1 = SLOT, B0 = 2 * SLOT, B1 = 3 * SLOT, A2 = 4 * SLOT;
  static constexpr int STG = B1;                        // epilogue staging: B1 | A2, 8 KiB per wave
  static constexpr int LDS = 5 * SLOT;                  // 163840
};

#define WAITV(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define WAITL0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

// SCORE (EPI_FC1 only): 0 none (evaluation passes), 1 pre-GELU, 2 post-GELU stage-1 score.  The scoring variant
// keeps the PLAIN operand order (lane <-> column, registers <-> rows): the per-(sample, neuron) sums of squares are then
// in-lane accumulations, and every partial sum is formed in exactly the order of gemm_bf16_kernel<EPI_FC1, SCORE>
// (a wave's 128 rows = that kernel's 128-row tile, passes h = 0, 1 = its row-waves), so the slab — and the stage-1
// scores — are bit-identical whichever kernel a launch is routed to.
// F8: both operands are e4m3 bytes (OCP fp8), 128 per 128-byte LDS row, so a K-tile carries K = 128 through the very same
// DMA pieces, ring slots and swizzle; the matrix instruction is v_mfma_scale_f32_32x32x64_f8f6f4 with unit block
// scales (twice the cycles of the bf16 32x32x16 form at four times the K: 2x the rate), 8 per unit instead of 16, fed by
// the same 12 ds_read_b128; the weight row's dequantisation scale is applied in the epilogue (acc * wscale[n] + bias).
// Which 32 of the 64 k-bytes a lane half supplies is free as long as both operands use one rule (lane half h takes
// bytes 32h .. 32h+31 of the 64-byte step, tools/fp8_probe.hip checks the pairing on the hardware).
// The kernel has two __global__ entry points over ONE body (gemm256_body.hip.h, included as text): gemm256_bf16_kernel<EPI, SCORE, F8> for
// the forms the project had before LayerScale, and gemm256_ls_kernel<F8> for EPI_RESID_LS.
template <int EPI, int SCORE = 0, bool F8 = false>
__global__ __launch_bounds__(512) void gemm256_bf16_kernel(const GemmArgs g) {
  static_assert(EPI != EPI_RESID_LS, "the LayerScale residual form is launched as gemm256_ls_kernel");
#include "gemm256_body.hip.h"
}
// EPI_RESID_LS (residual + LayerScale), bf16 or e4m3 operands, under an entry of its own: the ten forms above keep their names and their
// count; tests/test_layerscale_cpu.py holds these two to the same zero-scratch rule
template <bool F8 = false>
__global__ __launch_bounds__(512) void gemm256_ls_kernel(const GemmArgs g) {
  constexpr int EPI = EPI_RESID_LS, SCORE = 0;
#include "gemm256_body.hip.h"
}
// the entry point of a form (what a launch site takes the address of)
template <int EPI, int SCORE = 0, bool F8 = false>
static constexpr auto gemm256_entry() {
  if constexpr (EPI == EPI_RESID_LS) return &gemm256_ls_kernel<F8>;
  else return &gemm256_bf16_kernel<EPI, SCORE, F8>;
}
