// Key-streaming attention, d_h = 64, for sequences the resident kernels of attn.hip.h cannot hold (more than 288 tokens:
// 384-pixel /16 models with 577 tokens, patch-8 models with 785, ...).  bf16 in, bf16 (or, full form, e4m3) out, f32 accumulation,
// online softmax.
//
// Full form (attn64_stream_kernel): one 5-wave workgroup per (image, head, block of four 32-query tiles).  Waves 0..3 are the
// consumers (one query tile each), wave 4 is the producer: it streams K and V through LDS in stages of 128 keys (four 32-key
// tiles, 32 KiB of K + V), double-buffered, by LDS-DMA — the same lane-linear 1-KiB pieces and the same swizzles as
// attn64_persist_kernel (K chunk ^= (row >> 1) & 7 for ds_read_b128, V 64-byte half ^= (row >> 1) & 1 for ds_read_b64_tr_b16;
// a stage starts at a multiple of 128 keys, so the local row carries the global row's swizzle bits).  One s_barrier per stage:
//     producer:  [stage j landed: vmcnt(0)]  B(j)  issue stage j+1 -> buf[(j+1) & 1]
//     consumer:  [stage j-1 finished]        B(j)  stage j from buf[j & 1]
// buf[(j+1) & 1] held stage j-1, which every consumer finished before it arrived at B(j).  The producer's loop returns on its own,
// so no LDS-DMA lies on a consumer's control-flow path (no compiler-placed vmcnt wait in front of the consumers' LDS reads).
// Per stage a consumer computes S^T = K Q^T (lane <-> query, registers <-> keys, as in attn.hip.h), takes the stage maximum
// (in-lane + one half exchange), and updates the running state:
//     m' = max(m, max_stage s),  a = exp2((m - m') c2),  p = exp2(s c2 - m' c2),  l_lane = a l_lane + sum_lane p,  O^T = a O^T + V^T P^T
// with c2 = scale * log2 e (the scale folds into the exponent as in softmax_tile).  The rescale is applied on every stage (no deferred
// threshold): its cost is one v_exp and 16 packed multiplies per 128 keys.  The two lane halves' partial sums l_lane are exchanged
// once, at the end.  Keys past `tokens` of the last stage are -inf (p = 0); their K / V rows copy the last valid row (finite), and
// key tiles wholly past `tokens` are neither loaded nor multiplied.  Query rows past `tokens` are clamped and never stored.
// The output goes through a wave-private [32 queries][128 B] LDS tile (placed in the ring buffer the last stage does not use) as
// whole 128-byte row segments.
// OUT8 form (attn64_stream_kernel<true>, the fp8 mode's out-projection operand): the same main loop, and instead of the bf16 tile the
// e4m3(o * out8_scale) bytes of the fp32 accumulator, by the rule of attn64_persist_kernel: the wave's [32 queries][64 B] tile through
// the same staging slot (a lane's four consecutive d_h are one dword), then 128 sixteen-byte row pieces, two per lane; a wave that
// clipped a value adds 1 to *sat_counter.  No bf16 output is written.  attn64_stream_kernel<false> is the bf16 kernel as it was.
//
// CLS-only form (attn64_stream_cls_kernel<P>, the evaluation tail): P = 1 or 2 prefix queries per (image, head) against every key.  One
// wave per item, four items per workgroup: lane <-> key for the scores (chunks of 64 keys, online max / sum as above, f32 probabilities), then
// lane <-> d_h for P V (the chunk's probabilities broadcast by ds_bpermute).  q from the compact [n, q_img_stride] buffer, output to
// the compact [n, o_img_stride] buffer, as attn_fwd_kernel<64, NT, true>.
//
// The CLS-only form writes bf16 only (the evaluation tail stays bf16 in fp8 mode).  A streaming engine refuses fp8 unless
// SSP2_OPT_STREAM_FP8 is set; with it the full form feeds the e4m3 out-projection (SSP2_OPT_FP8_PROJ) as the persistent kernels do.
#pragma once
#include "attn.hip.h"          // attn_f32x2, the common helpers

#define ATTN_STREAM_MAX_TOKENS 8192      // largest sequence the streaming kernels (and ssp2_attention_stream_bf16) accept
#define ATTN_STREAM_QW 4                 // consumer waves = 32-query tiles per workgroup (the producer is wave ATTN_STREAM_QW)
#define ATTN_STREAM_KTS 4                // 32-key tiles per stage
#define ATTN_STREAM_STAGE (2 * ATTN_STREAM_KTS * 32 * 128)                 // K + V bytes of one stage
#define ATTN_STREAM_SMEM (2 * ATTN_STREAM_STAGE)                            // double-buffered ring (64 KiB)
static_assert(ATTN_STREAM_QW * 4096 <= ATTN_STREAM_STAGE, "the output staging tiles live in one ring buffer");

template <bool OUT8>
__global__ __launch_bounds__(64 * (ATTN_STREAM_QW + 1), 2) void attn64_stream_kernel(const bf16* __restrict__ qkv, int ld, bf16* __restrict__ out, int ldo,
                                                                                    int tokens, int dim, int heads, int qblocks, float scale, RowMap rm,
                                                                                    uint8_t* __restrict__ out8, int ldo8, unsigned int* __restrict__ sat_counter,
                                                                                    float out8_scale) {
  constexpr int QW = ATTN_STREAM_QW, KTS = ATTN_STREAM_KTS, SK = KTS * 32, KV = SK * 128, STAGE = ATTN_STREAM_STAGE;
  constexpr int KS = 4, DT = 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, lh = lane >> 5;
  // block -> (image, head, query block): the query blocks of one (image, head) are neighbours, so its K / V re-reads hit L2
  const int blk = blockIdx.x;
  const int item = blk / qblocks, qb = blk - item * qblocks;
  const int img = item / heads, head = item - img * heads;
  const size_t r0 = (size_t)row_of(rm, img);
  const bf16* const base = qkv + r0 * ld + head * 64;
  const int ns = (tokens + SK - 1) / SK;                        // stages

  if (wave == QW) {
    // ---- producer: key tiles with at least one valid key are loaded whole (rows past `tokens` copy the last valid row)
    const int c = lane & 7;
    auto issue = [&](int s, int b) {
      char* Kd = smem + b * STAGE;
      char* Vd = Kd + KV;
#pragma unroll
      for (int t = 0; t < KTS; ++t) {
        if (s * SK + t * 32 >= tokens) break;                   // wave-uniform
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int piece = t * 4 + p, lrow = piece * 8 + (lane >> 3), row = s * SK + lrow;
          const int rc = row < tokens ? row : tokens - 1;
          glds16(base + (size_t)rc * ld + dim + ((c ^ ((lrow >> 1) & 7)) << 3), Kd + piece * 1024);
          glds16(base + (size_t)rc * ld + 2 * dim + ((c ^ (((lrow >> 1) & 1) << 2)) << 3), Vd + piece * 1024);
        }
      }
    };
    issue(0, 0);
    for (int j = 0; j < ns; ++j) {
      asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
      if (j + 1 < ns) issue(j + 1, (j + 1) & 1);
    }
    return;
  }

  // ---- consumers
  const int qt = qb * QW + wave;
  const bool active = qt * 32 < tokens;                         // wave-uniform; an idle wave still meets every barrier
  bf16x8 qf[KS];
  {
    const int q = qt * 32 + l31;
    const int qc = q < tokens ? q : tokens - 1;
    const bf16* qp = base + (size_t)qc * ld + 8 * lh;
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = *(const bf16x8*)(qp + 16 * s);
  }
  const int tr_q = (lane & 15) >> 2, tr_p = lane & 3, tr_g = (lane >> 4) & 1;
  const int v_lane_off = (4 * lh + tr_q) * 128 + (16 * tr_g + 4 * tr_p) * 2;
  const int v_sw = (tr_q >> 1) & 1;
  const int k_sw = (l31 >> 1) & 7;
  const float c2 = scale * 1.44269504088896340736f;

  f32x16 oacc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[dt][i] = 0.f;
  float m_run = -INFINITY, l_lane = 0.f;

  for (int j = 0; j < ns; ++j) {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");     // this wave's reads of stage j-1 are done: its buffer may be refilled
    if (!active) continue;
    const char* Ks = smem + (j & 1) * STAGE;
    const char* Vs = Ks + KV;
    const int k0 = j * SK;
    const bool last = (j == ns - 1);
    f32x16 sacc[KTS];
#pragma unroll
    for (int kt = 0; kt < KTS; ++kt) {
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[kt][i] = 0.f;
      if (kt > 0 && last && k0 + kt * 32 >= tokens) {           // a key tile wholly past `tokens` (last stage only): not loaded
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[kt][i] = -INFINITY;
        continue;
      }
      const char* kp = Ks + (kt * 32 + l31) * 128;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const bf16x8 kf = *(const bf16x8*)(kp + (((2 * s + lh) ^ k_sw) << 4));
        sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], sacc[kt], 0, 0, 0);
      }
    }
    if (last) {                                                 // padding keys of the last stage -> -inf
#pragma unroll
      for (int kt = 0; kt < KTS; ++kt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = k0 + kt * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
          if (key >= tokens) sacc[kt][i] = -INFINITY;
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < KTS; ++kt)
#pragma unroll
      for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sacc[kt][i]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));                        // finite: every stage holds at least one valid key
    const float m_new = fmaxf(m_run, mx);
    const float mc = -m_new * c2;
    const float alpha = __builtin_amdgcn_exp2f(fmaf(m_run, c2, mc));     // first stage: exp2(-inf) = 0 (l and O are 0)
    m_run = m_new;
    attn_f32x2 c2v, mcv, sum2;
    c2v.x = c2v.y = c2; mcv.x = mcv.y = mc; sum2.x = sum2.y = 0.f;
#pragma unroll
    for (int kt = 0; kt < KTS; ++kt)
#pragma unroll
      for (int i = 0; i < 16; i += 2) {
        attn_f32x2 v; v.x = sacc[kt][i]; v.y = sacc[kt][i + 1];
        v = v * c2v + mcv;                                      // one v_pk_fma_f32
        attn_f32x2 e; e.x = __builtin_amdgcn_exp2f(v.x); e.y = __builtin_amdgcn_exp2f(v.y);
        sacc[kt][i] = e.x; sacc[kt][i + 1] = e.y;
        sum2 += e;                                              // one v_pk_add_f32
      }
    l_lane = fmaf(l_lane, alpha, sum2.x + sum2.y);
    attn_f32x2 av; av.x = av.y = alpha;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int i = 0; i < 16; i += 2) {
        attn_f32x2 o; o.x = oacc[dt][i]; o.y = oacc[dt][i + 1];
        o = o * av;                                             // one v_pk_mul_f32
        oacc[dt][i] = o.x; oacc[dt][i + 1] = o.y;
      }
#pragma unroll
    for (int kt = 0; kt < KTS; ++kt) {
      if (kt > 0 && last && k0 + kt * 32 >= tokens) continue;   // P = 0 there (and its V rows were not loaded)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        bf16x8 pf;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) pf[jj] = (bf16)sacc[kt][8 * s2 + jj];
        const char* vp = Vs + (kt * 32 + 16 * s2) * 128 + v_lane_off;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (__attribute__((address_space(3))) bf16x4*)(vp + (dt ^ v_sw) * 64));
          const bf16x4 v2 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (__attribute__((address_space(3))) bf16x4*)(vp + (dt ^ v_sw) * 64 + 8 * 128));
          bf16x8 vf;
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) { vf[jj] = v1[jj]; vf[4 + jj] = v2[jj]; }
          oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, oacc[dt], 0, 0, 0);
        }
      }
    }
  }
  if (!active) return;
  float l = l_lane + __shfl_xor(l_lane, 32);
  const float inv = 1.0f / l;
  // staging tile in the ring buffer the last stage did not use: it held stage ns - 2 (finished by every consumer before B(ns - 1))
  // or nothing, and the producer issues nothing after B(ns - 1)
  char* const ost = smem + (((ns - 1) & 1) ^ 1) * STAGE + wave * 4096;
  if constexpr (OUT8) {
    // e4m3 bytes (attn64_persist_kernel's rule): row q of the tile = 64 B at ost + q * 64, the lane's dword at d_h = 32 dt + 8 g4 + 4 lh
    const float sc8 = inv * out8_scale;
    bool sat8 = false;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
        *(uint32_t*)(ost + l31 * 64 + dt * 32 + 8 * g4 + 4 * lh) = pack_e4m3x4_sat(oacc[dt][4 * g4] * sc8, oacc[dt][4 * g4 + 1] * sc8,
                                                                                 oacc[dt][4 * g4 + 2] * sc8, oacc[dt][4 * g4 + 3] * sc8, sat8);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    f32x4 o8[2];
#pragma unroll
    for (int r2 = 0; r2 < 2; ++r2) o8[r2] = *(const f32x4*)(ost + (r2 * 64 + lane) * 16);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int r2 = 0; r2 < 2; ++r2) {
      const int c = r2 * 64 + lane, qq = qt * 32 + (c >> 2);
      if (qq < tokens) *(f32x4*)(out8 + (r0 + qq) * (size_t)ldo8 + head * 64 + (c & 3) * 16) = o8[r2];
    }
    report_sat(sat8, sat_counter);            // (padding queries repeat the last token's row: they cannot saturate alone)
    return;
  }
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      bf16x4 o4;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) o4[jj] = (bf16)(oacc[dt][4 * g4 + jj] * inv);
      *(bf16x4*)(ost + l31 * 128 + (((dt * 4 + g4) ^ (l31 & 7)) << 4) + lh * 8) = o4;
    }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  bf16x8 ov[4];
#pragma unroll
  for (int r4 = 0; r4 < 4; ++r4) {
    const int r = r4 * 8 + (lane >> 3);
    ov[r4] = *(const bf16x8*)(ost + r * 128 + (((lane & 7) ^ (r & 7)) << 4));
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int r4 = 0; r4 < 4; ++r4) {
    const int qq = qt * 32 + r4 * 8 + (lane >> 3);
    if (qq < tokens) *(bf16x8*)(out + (r0 + qq) * ldo + head * 64 + (lane & 7) * 8) = ov[r4];
  }
}

// CLS-only form: wave = one (image, head) item, 4 items per 256-thread workgroup (no LDS, no barrier).  P prefix queries per item
// (P = 1: CLS; P = 2: CLS and the distillation token, q and out prefix-major with the strides q_pstride / o_pstride): the P queries
// share every key and value load and keep P online-softmax states; for P = 1 the instruction sequence is the single-query one.
template <int P>
__global__ __launch_bounds__(256) void attn64_stream_cls_kernel(const bf16* __restrict__ qkv, int ld, const bf16* __restrict__ qsrc, size_t q_img_stride,
                                                                bf16* __restrict__ out, size_t o_img_stride, int tokens, int dim, int heads, int n_items,
                                                                float scale, RowMap rm, size_t q_pstride = 0, size_t o_pstride = 0) {
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (item >= n_items) return;                                  // wave-uniform
  const int img = item / heads, head = item - img * heads;
  const bf16* const base = qkv + (size_t)row_of(rm, img) * ld + head * 64;
  const float c2 = scale * 1.44269504088896340736f;
  float q[P][64];
#pragma unroll
  for (int t = 0; t < P; ++t) {
    const bf16* qp = qsrc + (size_t)t * q_pstride + (size_t)img * q_img_stride + head * 64;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const bf16x8 v = *(const bf16x8*)(qp + 8 * c);
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) q[t][8 * c + jj] = (float)v[jj];
    }
  }
  float m_run[P], l_lane[P], o[P];                              // o: output column d = lane
#pragma unroll
  for (int t = 0; t < P; ++t) { m_run[t] = -INFINITY; l_lane[t] = 0.f; o[t] = 0.f; }
  for (int k0 = 0; k0 < tokens; k0 += 64) {
    const int key = k0 + lane;
    const int kc = key < tokens ? key : tokens - 1;
    const bf16* kp = base + (size_t)kc * ld + dim;
    float s[P];
#pragma unroll
    for (int t = 0; t < P; ++t) s[t] = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const bf16x8 v = *(const bf16x8*)(kp + 8 * c);
#pragma unroll
      for (int jj = 0; jj < 8; ++jj)
#pragma unroll
        for (int t = 0; t < P; ++t) s[t] = fmaf((float)v[jj], q[t][8 * c + jj], s[t]);
    }
    float p[P];
#pragma unroll
    for (int t = 0; t < P; ++t) {
      if (key >= tokens) s[t] = -INFINITY;
      float mx = s[t];
#pragma unroll
      for (int w = 32; w >= 1; w >>= 1) mx = fmaxf(mx, __shfl_xor(mx, w));
      const float m_new = fmaxf(m_run[t], mx);
      const float mc = -m_new * c2;
      const float alpha = __builtin_amdgcn_exp2f(fmaf(m_run[t], c2, mc));
      m_run[t] = m_new;
      p[t] = __builtin_amdgcn_exp2f(fmaf(s[t], c2, mc));
      l_lane[t] = fmaf(l_lane[t], alpha, p[t]);
      o[t] *= alpha;
    }
    const int kn = tokens - k0 < 64 ? tokens - k0 : 64;        // valid keys of the chunk (wave-uniform)
    const bf16* vp = base + (size_t)k0 * ld + 2 * dim + lane;
    for (int kk = 0; kk < kn; ++kk) {
      const float v = (float)vp[(size_t)kk * ld];
#pragma unroll
      for (int t = 0; t < P; ++t) o[t] = fmaf(__shfl(p[t], kk), v, o[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < P; ++t) {
    float l = l_lane[t];
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) l += __shfl_xor(l, w);
    out[(size_t)t * o_pstride + (size_t)img * o_img_stride + head * 64 + lane] = (bf16)(o[t] / l);
  }
}
