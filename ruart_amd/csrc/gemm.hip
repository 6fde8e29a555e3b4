// Dense projections  C[M,N] = epilogue(A[M,K] . W[N,K]^T + bias[N]) [+ residual[M,N]]
//
// Replaces the nn.Linear sites of the reference's BERT encoder
//   Models/Bert/modeling.py:225-227 (Q,K,V), :261 (attention output dense),
//   :287-288 (intermediate dense + erf-GELU), :300 (output dense)
// with fused bias / GELU / residual epilogues (the residual add of :263 / :302 is folded in;
// the layer-norm itself is ruart_rows_layernorm).  Both operands are K-contiguous ("NT"),
// which is exactly the torch nn.Linear weight layout, so checkpoints load without a transpose.
//
//  * gemm_16_nt_128: bf16 or f16 operands, fp32 accumulate on v_mfma_f32_16x16x32_{bf16,f16} (same rate).
//    128x128x64 block tile, 4 waves (2x2), each wave 64x64 = 4x4 MFMA tiles.
//    LDS tiles are [128 rows][64 k] bf16 with the 16-byte chunk index XOR-swizzled by (row & 7),
//    which makes every ds_read_b128 fragment read conflict-free (cdna_hip_programming.md T2).
//    Register-staged double buffering: global loads for tile t+1 are issued before the MFMAs of
//    tile t and written to the other LDS buffer after them (T14 issue-early / write-late).
//    The MFMA is issued with W as the "A" operand and the activations as "B", so each lane ends
//    up with 4 consecutive output columns of one row -> 8/16-byte epilogue stores.
//    Workgroup ids are remapped XCD-aware with the N tile fastest, so the workgroups that share an
//    activation panel run on one XCD's L2.
//  * gemm_f32_nt_64: exact-fp32 path on v_mfma_f32_16x16x4_f32 (bitwise an fmaf chain), any M,N,K,
//    used for the fp32 validation mode and the small SDNet projections.
#include "common.h"
#include <type_traits>
#include "ruart_hip.h"
#include "gemm_shared.h"

#define BM 128
#define BN 128
#define BK 64

__device__ __forceinline__ float gelu_erf(float x) { return x * 0.5f * (1.0f + erff(x * 0.70710678118654752440f)); }

// erf for the 16-bit epilogue: Abramowitz-Stegun 7.1.26, |abs err| <= 1.5e-7 - far below the half-ulp of an f16/bf16
// output (>= 2.4e-4 relative) - at a third of erff's instruction count (the GELU epilogue runs on 3072-wide rows).
__device__ __forceinline__ float erf_as(float x) {
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));          // raw v_rcp_f32 (1 ulp), not an IEEE divide
  float p = fmaf(1.061405429f, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  const float e = __builtin_amdgcn_exp2f(ax * ax * -1.4426950408889634f);      // exp(-x^2) on v_exp_f32
  const float r = fmaf(-p * t, e, 1.0f);
  return copysignf(r, x);
}
__device__ __forceinline__ float gelu_fast(float x) { return x * 0.5f * (1.0f + erf_as(x * 0.70710678118654752440f)); }

template <typename T16, bool OUT_F32, int RES /*0 none, 1 same 16-bit type, 2 f32*/, int ACT /*0 none 1 gelu*/>
__global__ __launch_bounds__(256) void gemm_16_nt_128(const T16* __restrict__ A, int lda,
                                                      const T16* __restrict__ W, int ldw,
                                                      const float* __restrict__ bias, const void* __restrict__ R, int ldr,
                                                      void* __restrict__ C, int ldc, int M, int N, int K, int order) {
  constexpr int kTile = BM * BK * 2;             // bytes of one operand tile (16 KB)
  constexpr int kStage = 2 * kTile;              // A tile then W tile
  __shared__ __attribute__((aligned(1024))) char smem[2 * kStage];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int ntn = N / BN, ntm = M / BM;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  int tm, tn;
  tile_of(id, ntm, ntn, order, tm, tn);          // L2-friendly order inside an XCD's contiguous id range (gemm_shared.h)
  const int m0 = tm * BM, n0 = tn * BN;

  // Direct-to-LDS staging (global_load_lds_dwordx4): one wave-instruction fills 1 KB = 8 tile rows of 128 B.  The LDS
  // image is lane-linear, so the XOR swizzle is applied to the SOURCE chunk: lane l (row l>>3 of the 8, slot l&7)
  // fetches logical chunk (l&7) ^ (l>>3) (cdna_hip_programming.md rule 21: linear dest + swizzled source + swizzled read).
  const int srow = lane >> 3, schunk = (lane & 7) ^ srow;
  const T16* a_src = A + (size_t)(m0 + wave * 32 + srow) * lda + schunk * 8;
  const T16* w_src = W + (size_t)(n0 + wave * 32 + srow) * ldw + schunk * 8;
  const size_t a_step = (size_t)8 * lda, w_step = (size_t)8 * ldw;
  auto stage = [&](int buf, int k0) {
    char* base = smem + buf * kStage + wave * 4096;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __builtin_amdgcn_global_load_lds((gptr_t)(a_src + i * a_step + k0), (lptr_t)(base + i * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)(w_src + i * w_step + k0), (lptr_t)(base + kTile + i * 1024), 16, 0, 0);
    }
  };

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  typedef typename Vec8<T16>::type frag_t;
  auto compute = [&](int buf) {
    const char* sa = smem + buf * kStage;
    const char* sw = sa + kTile;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      frag_t wf[4], af[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        wf[i] = *reinterpret_cast<const frag_t*>(sw + lds_off(wn * 64 + i * 16 + fr, ks * 4 + fq));
        af[i] = *reinterpret_cast<const frag_t*>(sa + lds_off(wm * 64 + i * 16 + fr, ks * 4 + fq));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma_16x16x32(wf[i], af[j], acc[i][j]);
    }
  };

  const int nt = K / BK;
  stage(0, 0);
  __syncthreads();                  // (the compiler drains vmcnt before the barrier while an LDS-DMA is outstanding)
  for (int t = 0; t < nt - 1; ++t) {
    stage((t + 1) & 1, (t + 1) * BK);
    compute(t & 1);
    __syncthreads();
  }
  compute((nt - 1) & 1);

  // epilogue: acc[i][j][r] = C[m = m0+wm*64+j*16+fr][n = n0+wn*64+i*16+fq*4+r]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + wn * 64 + i * 16 + fq * 4;
    f32x4_t bv = {0.f, 0.f, 0.f, 0.f};
    if (bias) bv = *reinterpret_cast<const f32x4_t*>(bias + n);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + wm * 64 + j * 16 + fr;
      f32x4_t v = acc[i][j] + bv;
      if (ACT == 1) v = gelu4(v);
      if (RES == 1) v += load4(reinterpret_cast<const T16*>(R) + (size_t)m * ldr + n);
      if (RES == 2) v += load4(reinterpret_cast<const float*>(R) + (size_t)m * ldr + n);
      if (OUT_F32)
        store4(reinterpret_cast<float*>(C) + (size_t)m * ldc + n, v);
      else
        store4(reinterpret_cast<T16*>(C) + (size_t)m * ldc + n, v);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// 256x256x64 tile, 8 waves (2 along M x 4 along N, 128x64 per wave = 8x4 MFMA tiles, 128 accumulator VGPRs), two LDS
// stages of 64 KB, one workgroup per CU.  The 128x128 kernel is bound by how many bytes a CU can pull from L2 into LDS
// per unit time (PMC: ~36 GB/s/CU, MFMA pipe 24 % busy); this tile needs HALF the bytes per flop (128 flop/B), so the same
// byte rate feeds twice the MFMA work.  Same direct-to-LDS staging, source-side swizzle and fused epilogue.
// ------------------------------------------------------------------------------------------------
#define BM4 256
#define BN4 256
template <typename T16, bool OUT_F32, int RES, int ACT>
__global__ __launch_bounds__(512, 2) void gemm_16_nt_256sq(const T16* __restrict__ A, int lda, const T16* __restrict__ W, int ldw,
                                                           const float* __restrict__ bias, const void* __restrict__ R, int ldr,
                                                           void* __restrict__ C, int ldc, int M, int N, int K, int order) {
  constexpr int kTile = BM4 * BK * 2;            // 32 KB per operand tile
  constexpr int kStage = 2 * kTile;              // 64 KB
  extern __shared__ __attribute__((aligned(1024))) char smem[];   // 2 * kStage = 128 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int ntn = N / BN4, ntm = M / BM4;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  int tm, tn;
  tile_of(id, ntm, ntn, order, tm, tn);
  const int m0 = tm * BM4, n0 = tn * BN4;

  const int srow = lane >> 3, schunk = (lane & 7) ^ srow;
  const T16* a_src = A + (size_t)(m0 + wave * 32 + srow) * lda + schunk * 8;
  const T16* w_src = W + (size_t)(n0 + wave * 32 + srow) * ldw + schunk * 8;
  const size_t a_step = (size_t)8 * lda, w_step = (size_t)8 * ldw;
  auto stage = [&](int buf, int k0) {
    char* base = smem + buf * kStage + wave * 4096;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __builtin_amdgcn_global_load_lds((gptr_t)(a_src + i * a_step + k0), (lptr_t)(base + i * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)(w_src + i * w_step + k0), (lptr_t)(base + kTile + i * 1024), 16, 0, 0);
    }
  };

  f32x4_t acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fq = lane >> 4;
  typedef typename Vec8<T16>::type frag_t;
  auto compute = [&](int buf) {
    const char* sa = smem + buf * kStage;
    const char* sw = sa + kTile;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      frag_t wf[4], af[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) wf[i] = *reinterpret_cast<const frag_t*>(sw + lds_off(wn * 64 + i * 16 + fr, ks * 4 + fq));
#pragma unroll
      for (int j = 0; j < 8; ++j) af[j] = *reinterpret_cast<const frag_t*>(sa + lds_off(wm * 128 + j * 16 + fr, ks * 4 + fq));
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] = mfma_16x16x32(wf[i], af[j], acc[i][j]);
    }
  };

  const int nt = K / BK;
  stage(0, 0);
  __syncthreads();
  for (int t = 0; t < nt - 1; ++t) {
    stage((t + 1) & 1, (t + 1) * BK);
    compute(t & 1);
    __syncthreads();
  }
  compute((nt - 1) & 1);

  // Epilogue through LDS: the MFMA accumulator layout gives a lane 4 consecutive columns of 16 DIFFERENT rows, i.e. 64-byte
  // pieces of 16 cache lines per store instruction (PMC/TA-bound: 5x the line touches of a row-wise store).  Each wave parks
  // its 128x64 tile in its own 8.5 KB of the (now idle) staging memory, 32 rows at a time, and reads it back row-wise:
  // one instruction then covers 4 whole rows x 256 B (fp32) / 128 B (16-bit) for the residual load and the store alike.
  __syncthreads();                                   // every wave is done reading operand tiles
  constexpr int ERS = 272;                           // 64 fp32 + 16 B pad: conflict-free for both the b128 writes and reads
  char* my = smem + wave * (32 * ERS);               // 8.5 KB per wave, 32 rows per pass
  const int rrow = lane >> 4, rcol = (lane & 15) * 4;
  f32x4_t bv = {0.f, 0.f, 0.f, 0.f};
  const int ncol = n0 + wn * 64 + rcol;
  if (bias) bv = *reinterpret_cast<const f32x4_t*>(bias + ncol);
#pragma unroll
  for (int hh = 0; hh < 4; ++hh) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        *reinterpret_cast<f32x4_t*>(my + (j * 16 + fr) * ERS + (i * 16 + fq * 4) * 4) = acc[i][hh * 2 + j];
    // eight independent rows per pass, each stage over all eight before the next: the residual loads are all in flight
    // before the first LDS read returns, and the GELU chains (2 transcendentals deep) interleave instead of running back to back
    f32x4_t v[8], res[8];
    const int mrow = m0 + wm * 128 + hh * 32 + rrow;
    if (RES != 0) {
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        if (RES == 1) res[rr] = load4(reinterpret_cast<const T16*>(R) + (size_t)(mrow + rr * 4) * ldr + ncol);
        if (RES == 2) res[rr] = load4(reinterpret_cast<const float*>(R) + (size_t)(mrow + rr * 4) * ldr + ncol);
      }
    }
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) v[rr] = *reinterpret_cast<const f32x4_t*>(my + (rr * 4 + rrow) * ERS + rcol * 4) + bv;
    if (ACT == 1) {
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) v[rr] = gelu4(v[rr]);
    }
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
      if (RES != 0) v[rr] += res[rr];
      if (OUT_F32)
        store4(reinterpret_cast<float*>(C) + (size_t)(mrow + rr * 4) * ldc + ncol, v[rr]);
      else
        store4(reinterpret_cast<T16*>(C) + (size_t)(mrow + rr * 4) * ldc + ncol, v[rr]);
    }
  }
}

// Epilogue of one 256 x 256 tile of gemm_16_nt_256p8 through LDS, eight rows per pass; shared with the fix-up kernel of its split tail
// tiles (gemm_16_fixup).  `smem`: >= 8 x 32 x 272 bytes no wave reads as operand tiles any more.
// FK (round 6: the LayerNorms of the plain 16-bit pass folded into the projections, as the fp16c pass has had them since round 5 -
// CorrFold, gemm_shared.h): 0 none; 1 the A rows are pre-LayerNorm rows, v = rstd 2^s (acc - mu c) + d before the activation (`bias` = d);
// 3 (RES = 1) y = acc + bias + residual with the residual rows normalised on the way in when f.rs_part is given, written as T16, and
// the row's (sum, sumsq) of the fp32 y per 256-column tile -> f.out_part.
template <typename T16, bool OUT_F32, int RES, int ACT, int FK = 0>
__device__ __forceinline__ void p8_epilogue(f32x4_t (&acc)[4][8], char* smem, int m0, int n0, int tm, const float* __restrict__ bias,
                                            const void* __restrict__ R, int ldr, void* __restrict__ C, int ldc, int N,
                                            void* __restrict__ C2, float* __restrict__ colpart, int hh0 = 0, int hh1 = 4,
                                            const CorrFold& f = CorrFold{}) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 2, wn = wave & 3, fr = lane & 15, fq = lane >> 4;
  constexpr int ERS = 272;
  char* my = smem + wave * (32 * ERS);
  const int rrow = lane >> 4, rcol = (lane & 15) * 4;
  f32x4_t bv = {0.f, 0.f, 0.f, 0.f};
  const int ncol = n0 + wn * 64 + rcol;
  if (bias) bv = *reinterpret_cast<const f32x4_t*>(bias + ncol);
  f32x4_t colsum = {0.f, 0.f, 0.f, 0.f};
  f32x4_t cv = {0.f, 0.f, 0.f, 0.f}, gv = {1.f, 1.f, 1.f, 1.f}, ev = {0.f, 0.f, 0.f, 0.f};
  bool res_ln = false;
  float wsc = 1.f;
  if constexpr (FK == 1) {
    fold_row_stats(smem, f.in_part, f.in_np, m0, f.inv_h, f.eps);
    cv = *reinterpret_cast<const f32x4_t*>(f.colc + ncol);
    wsc = f.wscale;
  }
  if constexpr (FK == 3) {
    res_ln = f.rs_part != nullptr;
    if (res_ln) {
      fold_row_stats(smem, f.rs_part, f.rs_np, m0, f.inv_h, f.eps);
      gv = *reinterpret_cast<const f32x4_t*>(f.rs_g + ncol);
      ev = *reinterpret_cast<const f32x4_t*>(f.rs_b + ncol);
    }
  }
  const float2* rstat = reinterpret_cast<const float2*>(smem + kFoldStatsOff) + wm * 128 + rrow;
  float2* rpart = reinterpret_cast<float2*>(smem + kFoldPartOff) + wn * 256 + wm * 128 + rrow;
#pragma unroll
  for (int hh = 0; hh < 4; ++hh) {
    if (hh < hh0 || hh >= hh1) continue;           // (the fix-up kernel runs one 32-row pass per workgroup)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        *reinterpret_cast<f32x4_t*>(my + (j * 16 + fr) * ERS + (i * 16 + fq * 4) * 4) = acc[i][hh * 2 + j];
    // eight independent rows per pass, each stage over all eight before the next: the residual loads are all in flight
    // before the first LDS read returns, and the GELU chains (2 transcendentals deep) interleave instead of running back to back
    f32x4_t v[8], res[8];
    const int mrow = m0 + wm * 128 + hh * 32 + rrow;
    if (RES != 0) {
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        if (RES == 1) res[rr] = load4(reinterpret_cast<const T16*>(R) + (size_t)(mrow + rr * 4) * ldr + ncol);
        if (RES == 2) res[rr] = load4(reinterpret_cast<const float*>(R) + (size_t)(mrow + rr * 4) * ldr + ncol);
      }
    }
    if constexpr (FK == 1) {
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        const float2 st = rstat[hh * 32 + rr * 4];
        const f32x4_t a = *reinterpret_cast<const f32x4_t*>(my + (rr * 4 + rrow) * ERS + rcol * 4);
        const float sc = st.y * wsc;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[rr][r] = fmaf(sc, fmaf(-st.x, cv[r], a[r]), bv[r]);
      }
    } else {
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) v[rr] = *reinterpret_cast<const f32x4_t*>(my + (rr * 4 + rrow) * ERS + rcol * 4) + bv;
    }
    if constexpr (FK == 3) {
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        if (res_ln) {
          const float2 st = rstat[hh * 32 + rr * 4];
#pragma unroll
          for (int r = 0; r < 4; ++r) res[rr][r] = fmaf(gv[r], (res[rr][r] - st.x) * st.y, ev[r]);
        }
        v[rr] += res[rr];
        store4(reinterpret_cast<T16*>(C) + (size_t)(mrow + rr * 4) * ldc + ncol, v[rr]);
        const float s1 = row16_sum((v[rr][0] + v[rr][1]) + (v[rr][2] + v[rr][3]));
        const float s2 = row16_sum(fmaf(v[rr][0], v[rr][0], v[rr][1] * v[rr][1]) + fmaf(v[rr][2], v[rr][2], v[rr][3] * v[rr][3]));
        if ((lane & 15) == 0) rpart[hh * 32 + rr * 4] = make_float2(s1, s2);
      }
      continue;
    }
    if (ACT == 3) {
      // backward through the GELU (R = the f16 pre-activation H): C = acc * gelu'(H) - the gradient at the intermediate dense output -,
      // C2 = gelu(H) again (the X operand of the next weight gradient), colsum += this pass's rows of C before their rounding
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        const f32x4_t hv = load4(reinterpret_cast<const f16_t*>(R) + (size_t)(mrow + rr * 4) * ldr + ncol);
        f32x2_t g0, d0, g1, d1;
        gelu_fwd_bwd_pk((f32x2_t){hv[0], hv[1]}, g0, d0);
        gelu_fwd_bwd_pk((f32x2_t){hv[2], hv[3]}, g1, d1);
        v[rr] *= (f32x4_t){d0.x, d0.y, d1.x, d1.y};
        colsum += v[rr];
        store4(reinterpret_cast<T16*>(C2) + (size_t)(mrow + rr * 4) * ldc + ncol, (f32x4_t){g0.x, g0.y, g1.x, g1.y});
        store4(reinterpret_cast<T16*>(C) + (size_t)(mrow + rr * 4) * ldc + ncol, v[rr]);
      }
      continue;
    }
    if (ACT == 2) {                                          // training forward: the pre-activation is kept for the backward pass
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) store4(reinterpret_cast<T16*>(C2) + (size_t)(mrow + rr * 4) * ldc + ncol, v[rr]);
    }
    if (ACT != 0) {
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) v[rr] = gelu4(v[rr]);
    }
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
      if (RES != 0) v[rr] += res[rr];
      if (OUT_F32)
        store4(reinterpret_cast<float*>(C) + (size_t)(mrow + rr * 4) * ldc + ncol, v[rr]);
      else
        store4(reinterpret_cast<T16*>(C) + (size_t)(mrow + rr * 4) * ldc + ncol, v[rr]);
    }
  }
  if constexpr (FK == 3) {
    // the four column groups of a row in a fixed order -> this tile's partial of the row (as gemm_corr.hip's kind 3)
    __syncthreads();
    if (threadIdx.x < 256) {
      const float2* pp = reinterpret_cast<const float2*>(smem + kFoldPartOff) + threadIdx.x;
      const float2 a = pp[0], b = pp[256], c = pp[512], d = pp[768];
      reinterpret_cast<float2*>(f.out_part)[(size_t)(m0 + threadIdx.x) * kFoldSlots + n0 / 256] = make_float2((a.x + b.x) + (c.x + d.x), (a.y + b.y) + (c.y + d.y));
    }
  }
  if (ACT == 3 && colpart) {
    // the wave's 128 rows: lanes l, l + 16, l + 32, l + 48 hold the same four columns
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      colsum[r] += __shfl_xor(colsum[r], 16, 64);
      colsum[r] += __shfl_xor(colsum[r], 32, 64);
    }
    if (lane < 16) store4(colpart + (size_t)(tm * 2 + wm) * N + ncol, colsum);
  }
}

// ------------------------------------------------------------------------------------------------
// 256x256x64, four phases per K-tile with the prefetch in flight ACROSS barriers (the "8-phase" schedule of the CDNA4
// playbook: 2 K-tiles = 8 phases per loop iteration).  Same tile, wave layout, swizzle and epilogue as gemm_16_nt_256sq.
//
//  * Each operand K-tile is staged as two half-tiles of 128 rows (16 KB, two global_load_lds per thread).  Half h of A holds,
//    for BOTH wave rows wm, rows wm*128 + h*64 .. +64; half h of W holds, for every wave column wn, rows wn*64 + h*32 .. +32.
//    So every wave reads its first 64x32 quadrant operands from halves 0, and a half-tile is dead for ALL waves at a known
//    phase:  W-h0 after phase 0 (its 4 reads are retired by lgkmcnt(8) before phase 0's first barrier), A-h0 after phase 0,
//    W-h1 after phase 1, A-h1 after phase 2.
//  * Phase p of K-tile t:  ds_read the fragments the quadrant needs | issue ONE half-tile prefetch | s_barrier |
//    lgkmcnt(0) | 16 MFMA (one 64x32 quadrant x K=64) | s_barrier.  Prefetch order: phase 0 -> (t+1, A-h1); phase 1 ->
//    (t+2, W-h0); phase 2 -> (t+2, A-h0); phase 3 -> (t+2, W-h1): every slot is restaged >= 2 phases after its last read
//    (1 phase for W-h0, whose reads were retired before the barrier).
//  * vmcnt is counted, never 0 in the steady state: phase 3 waits vmcnt(6) = the three youngest half-tiles stay in flight
//    across the barriers, everything older - all of K-tile t+1 - has landed; it is read one phase later (after a barrier every
//    wave passed following its own wait).
//  * Waves 4-7 (wm = 1) run one barrier behind waves 0-3: while one group issues MFMAs the other does its LDS reads and
//    prefetch issue, so each SIMD's matrix pipe alternates between its two resident waves instead of idling while both read.
// Needs K % 128 == 0 (even number of K-tiles), M % 256 == 0, N % 256 == 0.
// ------------------------------------------------------------------------------------------------
template <typename T16, bool OUT_F32, int RES, int ACT, int FK = 0>
__global__ __launch_bounds__(512, 2) void gemm_16_nt_256p8(const T16* __restrict__ A, int lda, const T16* __restrict__ W, int ldw,
                                                           const float* __restrict__ bias, const void* __restrict__ R, int ldr,
                                                           void* __restrict__ C, int ldc, int M, int N, int K, int order, int kchunk,
                                                           void* __restrict__ C2, float* __restrict__ colpart, int n_full, int S,
                                                           float* __restrict__ slabs, const CorrFold fold) {
  if (kchunk > 0) {
    // split-K form (weight gradients: small output, K = all token rows): slice blockIdx.y multiplies columns [z * kchunk, ...) of
    // both operands and writes its own fp32 slab z of C; ruart_splitk_reduce adds the slabs in slice order
    const int z = blockIdx.y;
    A += (size_t)z * kchunk;
    W += (size_t)z * kchunk;
    K = min(kchunk, K - z * kchunk);
    C = reinterpret_cast<float*>(C) + (size_t)z * M * ldc;
  }
  constexpr int kHalf = 128 * BK * 2;            // 16 KB half-tile
  constexpr int kOper = 2 * kHalf;               // 32 KB per operand K-tile
  constexpr int kBuf = 2 * kOper;                // 64 KB per K-tile
  extern __shared__ __attribute__((aligned(1024))) char smem[];   // 2 * kBuf = 128 KB, the ONLY LDS object
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: wave-dependent offsets stay in SGPRs
  const int wm = wave >> 2, wn = wave & 3;
  const int ntn = N / BN4, ntm = M / BM4;
  // A whole tile, or - the tail split of the launcher (tail_plan, gemm_shared.h) - one of the S K slices of a last tile, each over
  // nt / S K-tiles, parking its partial sums in `slabs` for gemm_16_fixup.  n_full == gridDim.x: no split (every other caller).
  int id, slice;
  tail_decode(blockIdx.x, n_full, S, id, slice);
  int tm, tn;
  tile_of(id, ntm, ntn, order, tm, tn);
  tm = __builtin_amdgcn_readfirstlane(tm);
  tn = __builtin_amdgcn_readfirstlane(tn);
  const int m0 = tm * BM4, n0 = tn * BN4;

  // staging: wave w fills local rows 16w .. 16w+15 of a half-tile (two 1 KB pieces of 8 rows x 128 B, lane-linear)
  // Addresses = uniform 64-bit base (SGPR pair) + ONE 32-bit per-lane byte offset per operand (dma16: the saddr form of global_load_lds).
  const int srow = lane >> 3, schunk = (lane & 7) ^ srow;
  const unsigned a_lane = (unsigned)(srow * lda + schunk * 8) * 2, w_lane = (unsigned)(srow * ldw + schunk * 8) * 2;      // bytes
  const T16* a_src = A + (size_t)(m0 + (wave >> 2) * 128 + (wave & 3) * 16) * lda;
  const T16* w_src = W + (size_t)(n0 + (wave >> 1) * 64 + (wave & 1) * 16) * ldw;
  const size_t a8 = (size_t)8 * lda, w8 = (size_t)8 * ldw, a_h = (size_t)64 * lda, w_h = (size_t)32 * ldw;
  char* const st_base = smem + wave * 2048;
  auto stage_a = [&](int d, int h, int kt) {
    char* dst = st_base + d * kBuf + h * kHalf;
    const T16* src = a_src + h * a_h + kt * BK;
    dma16(src, a_lane, dst);
    dma16(src + a8, a_lane, dst + 1024);
  };
  auto stage_w = [&](int d, int h, int kt) {
    char* dst = st_base + d * kBuf + kOper + h * kHalf;
    const T16* src = w_src + h * w_h + kt * BK;
    dma16(src, w_lane, dst);
    dma16(src + w8, w_lane, dst + 1024);
  };

  f32x4_t acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fq = lane >> 4;
  typedef typename Vec8<T16>::type frag_t;
  frag_t af[4][2], wf0[2][2], wf1[2][2];
  // (k-step outer: LDS returns in order, and the first eight MFMAs of a quadrant need only the ks = 0 fragments)
  auto read_a = [&](int d, int h) {
    const char* sa = smem + d * kBuf + h * kHalf;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 4; ++j) af[j][ks] = *reinterpret_cast<const frag_t*>(sa + lds_off(wm * 64 + j * 16 + fr, ks * 4 + fq));
  };
  auto read_w = [&](int d, int h, frag_t (&wf)[2][2]) {
    const char* sw = smem + d * kBuf + kOper + h * kHalf;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) wf[i][ks] = *reinterpret_cast<const frag_t*>(sw + lds_off(wn * 32 + i * 16 + fr, ks * 4 + fq));
  };
  // 16 MFMAs of one quadrant.  (Issuing the phase's prefetch between them instead of in the read segment measured 4 % SLOWER on the
  // BERT shapes and 2.5 % slower at 4096^3.)
  auto quad = [&](int hc, int hr, frag_t (&wf)[2][2]) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[hc * 2 + i][hr * 4 + j] = mfma_16x16x32(wf[i][ks], af[j][ks], acc[hc * 2 + i][hr * 4 + j]);
    }
    __builtin_amdgcn_s_setprio(0);
  };
  // one K-tile = four phases.  D: LDS buffer of this tile; N1: K-tile t+1 exists; N2: K-tile t+2 exists.
  // The read balancing that gemm_tn.hip ships measures neutral here (layer average 728 us against 724 us over three interleaved runs of
  // tools/gemm_corr_bench.py), and so does dropping the full LDS wait behind each phase's first barrier (712-721 vs 716 us per layer).
  auto tile = [&](auto dtag, auto n1tag, auto n2tag, int t) {
    constexpr int D = decltype(dtag)::value;
    constexpr bool N1 = decltype(n1tag)::value, N2 = decltype(n2tag)::value;
    // phase 0: quadrant (rows h0, cols h0); prefetch (t+1, A-h1)
    read_w(D, 0, wf0);
    __builtin_amdgcn_sched_barrier(0);
    read_a(D, 0);
    if (N1) stage_a(D ^ 1, 1, t + 1);
    asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");     // the 4 W-h0 reads (issued first) are back: its slot may be restaged
    RUART_BAR();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    quad(0, 0, wf0);
    RUART_BAR();
    // phase 1: (rows h0, cols h1); prefetch (t+2, W-h0)
    read_w(D, 1, wf1);
    if (N2) stage_w(D, 0, t + 2);
    RUART_BAR();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    quad(1, 0, wf1);
    RUART_BAR();
    // phase 2: (rows h1, cols h1); prefetch (t+2, A-h0)
    read_a(D, 1);
    if (N2) stage_a(D, 0, t + 2);
    RUART_BAR();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    quad(1, 1, wf1);
    RUART_BAR();
    // phase 3: (rows h1, cols h0) - operands already in registers; prefetch (t+2, W-h1)
    if (N2) {
      stage_w(D, 1, t + 2);
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");     // K-tile t+1 complete; the 3 youngest half-tiles stay in flight
    } else if (N1) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // last prefetch: (t+1, A-h1) from phase 0
    }
    RUART_BAR();
    quad(0, 1, wf0);
    RUART_BAR();
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using Tt = std::true_type;
  using Ff = std::false_type;

  const int nt = K / BK;                         // even, >= 2
  int kb = 0, ke = nt;                           // K-tiles of this workgroup: all, or slice `slice` of S (nt / S even, >= 2)
  if (slice >= 0) {
    const int L = __builtin_amdgcn_readfirstlane(nt / S);
    kb = slice * L;
    ke = kb + L;
  }
  stage_w(0, 0, kb);
  stage_a(0, 0, kb);
  stage_w(0, 1, kb);
  stage_a(0, 1, kb);
  stage_w(1, 0, kb + 1);
  stage_a(1, 0, kb + 1);
  stage_w(1, 1, kb + 1);
  asm volatile("s_waitcnt vmcnt(6)" ::: "memory");           // K-tile kb landed (this wave's share)
  RUART_BAR();
  if (wave >= 4) RUART_BAR();   // stagger: waves 4-7 run one barrier behind
  int t = kb;
  for (; t + 2 < ke; t += 2) {
    tile(I0{}, Tt{}, Tt{}, t);
    tile(I1{}, Tt{}, Tt{}, t + 1);
  }
  tile(I0{}, Tt{}, Ff{}, t);
  tile(I1{}, Ff{}, Ff{}, t + 1);
  if (wave < 4) RUART_BAR();    // waves 0-3 pair the lagging group's last barrier
  RUART_BAR();                                                  // every wave is done reading operand tiles

  if (slice >= 0) {
    tail_store_slab(slabs, id - n_full, S, slice, acc);
    return;
  }
  p8_epilogue<T16, OUT_F32, RES, ACT, FK>(acc, smem, m0, n0, tm, bias, R, ldr, C, ldc, N, C2, colpart, 0, 4, fold);
}

// ------------------------------------------------------------------------------------------------
// exact fp32 path: 64x64x16 tile, 4 waves (2x2) of 32x32, v_mfma_f32_16x16x4_f32
// ------------------------------------------------------------------------------------------------
#define FBM 64
#define FBN 64
#define FBK 16
#define FLD 17   // padded LDS row stride (floats): (17 r + k) mod 32 is conflict-free for ds_read_b32

template <bool VEC>
__global__ __launch_bounds__(256) void gemm_f32_nt_64(const float* __restrict__ A, int lda, const float* __restrict__ W, int ldw,
                                                      const float* __restrict__ bias, const float* __restrict__ R, int ldr,
                                                      float* __restrict__ C, int ldc, int M, int N, int K, int act) {
  __shared__ float As[FBM * FLD];
  __shared__ float Bs[FBN * FLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int ntn = (N + FBN - 1) / FBN;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (id / ntn) * FBM, n0 = (id % ntn) * FBN;
  const int lr = tid >> 2, lk = (tid & 3) * 4;       // staging: row 0..63, k 0/4/8/12

  auto gload = [&](const float* P, int ld, int row, int rows, int k0, float (&v)[4]) {
    const int kk = k0 + lk;
    if (row < rows) {
      const float* p = P + (size_t)row * ld + kk;
      if (VEC && kk + 3 < K) {
        f32x4_t t = *reinterpret_cast<const f32x4_t*>(p);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (kk + i < K) ? p[i] : 0.f;
      }
    } else {
      v[0] = v[1] = v[2] = v[3] = 0.f;
    }
  };

  f32x4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  float ra[4], rb[4];
  gload(A, lda, m0 + lr, M, 0, ra);
  gload(W, ldw, n0 + lr, N, 0, rb);
  const int fr = lane & 15, fq = lane >> 4;
  const int nt = (K + FBK - 1) / FBK;
  for (int t = 0; t < nt; ++t) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      As[lr * FLD + lk + i] = ra[i];
      Bs[lr * FLD + lk + i] = rb[i];
    }
    __syncthreads();
    if (t + 1 < nt) {
      gload(A, lda, m0 + lr, M, (t + 1) * FBK, ra);
      gload(W, ldw, n0 + lr, N, (t + 1) * FBK, rb);
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      float wf[2], af[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        wf[i] = Bs[(wn * 32 + i * 16 + fr) * FLD + kk * 4 + fq];
        af[i] = As[(wm * 32 + i * 16 + fr) * FLD + kk * 4 + fq];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i], af[j], acc[i][j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int n = n0 + wn * 32 + i * 16 + fq * 4;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int m = m0 + wm * 32 + j * 16 + fr;
      if (m >= M) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (n + r >= N) continue;
        float v = acc[i][j][r];
        if (bias) v += bias[n + r];
        if (act == 1) v = gelu_erf(v);
        else if (act == 2) v = fmaxf(v, 0.f);
        if (R) v += R[(size_t)m * ldr + n + r];
        C[(size_t)m * ldc + n + r] = v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// ---- optional live profiling of the dominant kernel (bench.py roofline): hipEvent pair around every 16-bit GEMM launch
#include <vector>
namespace {
struct ProfRec { hipEvent_t a, b; double flops; };
std::vector<ProfRec> g_prof_pool;
size_t g_prof_used = 0;
bool g_prof_on = false;
bool g_prof_marks_only = false;      // ruart_prof_enable(2): markers are recorded, the GEMM launches are not bracketed
}  // namespace
int g_tile_order = 8;            // GROUP_M of the tile walk (0 = plain row-major); tuning knob, see ruart_gemm_set_tile_order
int g_tile_order_auto = 1;       // the fp16c kernel picks GROUP_M per shape until ruart_gemm_set_tile_order is called (gemm_corr.hip)
int ruart_prof_real_rows = 0;   // set by ruart_bert_forward: algorithmic row count (the GEMM itself runs on padded rows)

extern int g_gemm_variant;
extern "C" int ruart_gemm_set_tile_order(int group_m) {
  RUART_ENTRY();
  if (group_m < -1 || group_m > 64) return (int)hipErrorInvalidValue;
  if (group_m < 0) {                 // -1: back to the per-problem rule (ruart_tile_group_m)
    g_tile_order = 8;
    g_tile_order_auto = 1;
    return 0;
  }
  g_tile_order = group_m;
  g_tile_order_auto = 0;
  return 0;
}
extern "C" int ruart_gemm_set_variant(int v) {
  RUART_ENTRY();
  if (v != 0 && v != 3 && v != 5 && v != 7) return (int)hipErrorInvalidValue;
  g_gemm_variant = v;
  return 0;
}

extern "C" int ruart_prof_enable(int on) {
  RUART_ENTRY();
  if (on && g_prof_pool.empty()) {
    g_prof_pool.resize(8192);
    for (auto& r : g_prof_pool) {
      if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return (int)hipErrorOutOfMemory;
    }
  }
  g_prof_on = on != 0;
  g_prof_marks_only = on == 2;
  g_prof_used = 0;
  return 0;
}

// shared with gemm_corr.hip: bracket one launch of an encoder GEMM (NULL when profiling is off)
void* ruart_prof_begin_(hipStream_t s, int M, int N, int K) {
  if (!g_prof_on || g_prof_marks_only || g_prof_used >= g_prof_pool.size()) return nullptr;
  ProfRec* rec = &g_prof_pool[g_prof_used++];
  const int rows = (ruart_prof_real_rows > 0 && ruart_prof_real_rows <= M) ? ruart_prof_real_rows : M;
  rec->flops = 2.0 * rows * (double)N * K;
  hipEventRecord(rec->a, s);
  return rec;
}
void ruart_prof_end_(void* rec, hipStream_t s) {
  if (rec) hipEventRecord(((ProfRec*)rec)->b, s);
}

// Diagnostics (tools/step_timeline.py): a marker record on any stream (flops = -tag) and the recorded launches' begin / end times in ms
// relative to the first record - one time base for the encoder's GEMM launches and for points of the step stream.
extern "C" int ruart_prof_mark(int tag, void* stream) {
  RUART_ENTRY();
  if (!g_prof_on || g_prof_used >= g_prof_pool.size()) return 0;
  ProfRec* rec = &g_prof_pool[g_prof_used++];
  rec->flops = -(double)tag;
  hipEventRecord(rec->a, (hipStream_t)stream);
  hipEventRecord(rec->b, (hipStream_t)stream);
  return 0;
}
extern "C" int ruart_prof_timeline(float* begin_ms, float* end_ms, double* flops, int max_records, int* n_records) {
  RUART_ENTRY();
  if (!begin_ms || !end_ms || !flops || !n_records) return (int)hipErrorInvalidValue;
  int n = 0;
  for (size_t i = 0; i < g_prof_used && n < max_records; ++i, ++n) {
    hipError_t e = hipEventSynchronize(g_prof_pool[i].b);
    if (e != hipSuccess) return (int)e;
    if ((e = hipEventElapsedTime(&begin_ms[n], g_prof_pool[0].a, g_prof_pool[i].a)) != hipSuccess) return (int)e;
    if ((e = hipEventElapsedTime(&end_ms[n], g_prof_pool[0].a, g_prof_pool[i].b)) != hipSuccess) return (int)e;
    flops[n] = g_prof_pool[i].flops;
  }
  *n_records = n;
  return 0;
}

extern "C" int ruart_prof_read(double* total_ms, long long* launches, double* flops) {
  RUART_ENTRY();
  double ms = 0.0, fl = 0.0;
  for (size_t i = 0; i < g_prof_used; ++i) {
    float t = 0.f;
    hipError_t e = hipEventSynchronize(g_prof_pool[i].b);
    if (e != hipSuccess) return (int)e;
    if ((e = hipEventElapsedTime(&t, g_prof_pool[i].a, g_prof_pool[i].b)) != hipSuccess) return (int)e;
    ms += t;
    fl += g_prof_pool[i].flops;
  }
  *total_ms = ms;
  *launches = (long long)g_prof_used;
  *flops = fl;
  g_prof_used = 0;
  return 0;
}

int g_gemm_variant = 5;          // 0: 128x128 2-stage (any M, N multiple of 128); 3: 256x256 2-stage; 5: 256x256 four phases per K-tile, counted
                                 // vmcnt, staggered wave groups (M, N % 256 == 0, K % 128 == 0; else 3, else 0)

// ------------------------------------------------------------------------------------------------
// Variant 7 (round 4 experiment, the verdict's form (b)): ONE wave per SIMD.  256x256x64 tile, 4 waves (2 x 2), each wave a 128x128 block =
// 8 x 8 MFMA tiles (256 accumulator registers; the kernel runs in the 512-register budget of a one-wave-per-SIMD launch).  Per MFMA the wave
// reads 1/4 fragment instead of the 3/8 of the 8-wave kernel (a third fewer LDS bytes), there is ONE workgroup barrier per K-tile instead of
// eight and no hand-over of the matrix pipe between two waves - but nobody else issues the wave's LDS-DMA and fragment reads: they sit
// between its own MFMAs (one ds_read_b128 per 4 MFMAs, one DMA per 8 in the second half of a K-tile).
//   K-tile t lives in LDS buffer t & 1 ([256 rows][128 B] per operand, the XOR swizzle of lds_off on the source chunk and on the read).
//   step 0 (k 0..31):  64 MFMAs on fragment set X | reads set Y = (t, k 32..63) from buffer b
//   mid-tile:          vmcnt(0) (this wave's pieces of tile t+1, issued one step ago, have landed), lgkmcnt(0), s_barrier
//                      -> buffer b is read by no wave any more, buffer b^1 is complete for every wave
//   step 1 (k 32..63): 64 MFMAs on set Y | reads set X = (t+1, k 0..31) from buffer b^1 | issues tile t+2's 16 DMA pieces into buffer b
// M, N % 256 == 0, K % 64 == 0, K >= 128.
// ------------------------------------------------------------------------------------------------
// MFMA with the accumulator tile pinned to the AGPR half of the register file ("+a"): with 256 accumulator registers plus two fragment
// sets the kernel needs > 256 registers, and left to itself hipcc (ROCm 7.2) keeps the MFMAs on VGPR accumulators and shuttles every tile
// through v_accvgpr_read / _write around each MFMA (4 + 4 vector moves per MFMA in the K loop).  The hazard recogniser does not see
// inside an asm statement: the accumulators are first read ~100 instructions and two barriers after the last MFMA (epilogue).
__device__ __forceinline__ void mfma_agpr(const f16x8_t& a, const f16x8_t& b, f32x4_t& c) {
  asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma_agpr(const bf16x8_t& a, const bf16x8_t& b, f32x4_t& c) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}

template <typename T16, bool OUT_F32, int RES, int ACT>
__global__ __launch_bounds__(256, 1) void gemm_16_nt_256w4(const T16* __restrict__ A, int lda, const T16* __restrict__ W, int ldw,
                                                           const float* __restrict__ bias, const void* __restrict__ R, int ldr,
                                                           void* __restrict__ C, int ldc, int M, int N, int K, int order) {
  constexpr int kOper = 256 * BK * 2;            // 32 KB per operand K-tile
  constexpr int kBuf = 2 * kOper;                // 64 KB per K-tile
  extern __shared__ __attribute__((aligned(1024))) char smem[];   // 2 * kBuf = 128 KB
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  int tm, tn;
  tile_of(__builtin_amdgcn_readfirstlane(xcd_remap(blockIdx.x, gridDim.x)), M / BM4, N / BN4, order, tm, tn);
  tm = __builtin_amdgcn_readfirstlane(tm);
  tn = __builtin_amdgcn_readfirstlane(tn);
  const int m0 = tm * BM4, n0 = tn * BN4;

  // staging: wave w fills rows 64 w .. 64 w + 63 of both operand tiles: 8 pieces of 8 rows x 128 B each
  const int srow = lane >> 3, schunk = (lane & 7) ^ srow;
  const unsigned a_lane = (unsigned)(srow * lda + schunk * 8) * 2, w_lane = (unsigned)(srow * ldw + schunk * 8) * 2;
  const T16* a_src = A + (size_t)(m0 + wave * 64) * lda;
  const T16* w_src = W + (size_t)(n0 + wave * 64) * ldw;
  const size_t a8 = (size_t)8 * lda, w8 = (size_t)8 * ldw;
  char* const st_base = smem + wave * 8192;
  auto piece = [&](int d, int q, int kt) {       // piece q of 16: 0..7 activations, 8..15 weights
    if (q < 8) dma16(a_src + (size_t)q * a8 + kt * BK, a_lane, st_base + d * kBuf + q * 1024);
    else dma16(w_src + (size_t)(q - 8) * w8 + kt * BK, w_lane, st_base + d * kBuf + kOper + (q - 8) * 1024);
  };

  f32x4_t acc[8][8];                             // [i: 16 columns of the wave's 128][j: 16 rows]
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fq = lane >> 4;
  typedef typename Vec8<T16>::type frag_t;
  frag_t fx[16], fy[16];                         // a fragment set: [0..7] weights (columns), [8..15] activations (rows)
  auto rd = [&](frag_t (&f)[16], int q, int d, int ks) {      // read q of 16 of the set for k-step ks of buffer d
    const char* base = smem + d * kBuf + (q < 8 ? kOper : 0);
    const int row = (q < 8 ? wn * 128 + q * 16 : wm * 128 + (q - 8) * 16) + fr;
    f[q] = *reinterpret_cast<const frag_t*>(base + lds_off(row, ks * 4 + fq));
  };
  // one k-step: 64 MFMAs on `cur`; behind every group of four, one read of `nxt` (buffer rd_d, k-step rd_ks; the eight activation
  // fragments first - the next step's first eight MFMAs need them all -, then the weight fragments in the order the MFMAs take them) and,
  // in the second half of a K-tile, one DMA piece of tile dma_kt into buffer dma_d.  sched_barrier pins the groups; RD / DMA are
  // compile-time so that no read or DMA sits behind a branch.
  auto step = [&](frag_t (&cur)[16], frag_t (&nxt)[16], auto rd_tag, int rd_d, int rd_ks, auto dma_tag, int dma_d, int dma_kt) {
    constexpr bool RD = decltype(rd_tag)::value, DMA = decltype(dma_tag)::value;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = g * 4 + u, i = idx >> 3, j = idx & 7;
        mfma_agpr(cur[i], cur[8 + j], acc[i][j]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (RD) rd(nxt, g < 8 ? 8 + g : g - 8, rd_d, rd_ks);
      if (DMA) piece(dma_d, g, dma_kt);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  using Tt = std::true_type;
  using Ff = std::false_type;
  auto mid = [&] {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the next tile's pieces (issued during the previous step 1 / the prologue)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    RUART_BAR();
    __builtin_amdgcn_sched_barrier(0);
  };
  auto end_step = [&] {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };

  const int nt = K / BK;                                      // >= 2
#pragma unroll
  for (int q = 0; q < 16; ++q) piece(0, q, 0);
#pragma unroll
  for (int q = 0; q < 16; ++q) piece(1, q, 1);
  asm volatile("s_waitcnt vmcnt(16)" ::: "memory");           // K-tile 0 landed (this wave's pieces)
  RUART_BAR();
#pragma unroll
  for (int q = 0; q < 16; ++q) rd(fx, q, 0, 0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  int t = 0;
  for (; t + 2 < nt; ++t) {                                   // tiles with two successors
    const int d = t & 1;
    step(fx, fy, Tt{}, d, 1, Ff{}, 0, 0);                     // step 0: compute (t, 0), read (t, 1)
    mid();
    step(fy, fx, Tt{}, d ^ 1, 0, Tt{}, d, t + 2);             // step 1: compute (t, 1), read (t+1, 0), stage t+2 into this tile's buffer
    end_step();
  }
  {                                                           // second to last tile: nothing left to stage
    const int d = t & 1;
    step(fx, fy, Tt{}, d, 1, Ff{}, 0, 0);
    mid();
    step(fy, fx, Tt{}, d ^ 1, 0, Ff{}, 0, 0);
    end_step();
    ++t;
  }
  {                                                           // last tile
    const int d = t & 1;
    step(fx, fy, Tt{}, d, 1, Ff{}, 0, 0);
    end_step();
    step(fy, fx, Ff{}, 0, 0, Ff{}, 0, 0);
  }
  RUART_BAR();                                                // every wave is done reading operand tiles
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");         // (MFMA results in AGPRs: the asm MFMAs are invisible to the hazard recogniser)

  // epilogue through LDS: 32 rows x 128 columns per wave and pass (528-byte rows: conflict-free for the 16-byte writes and reads)
  constexpr int ERS = 528;
  char* my = smem + wave * (32 * ERS);
  const int ncol = n0 + wn * 128 + (lane & 31) * 4;
  f32x4_t bv = {0.f, 0.f, 0.f, 0.f};
  if (bias) bv = *reinterpret_cast<const f32x4_t*>(bias + ncol);
#pragma unroll
  for (int hh = 0; hh < 4; ++hh) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
        *reinterpret_cast<f32x4_t*>(my + (jj * 16 + fr) * ERS + (i * 16 + fq * 4) * 4) = acc[i][hh * 2 + jj];
    f32x4_t v[16], res[16];
    const int mrow = m0 + wm * 128 + hh * 32 + (lane >> 5);
    if (RES != 0) {
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) {
        if (RES == 1) res[rr] = load4(reinterpret_cast<const T16*>(R) + (size_t)(mrow + rr * 2) * ldr + ncol);
        if (RES == 2) res[rr] = load4(reinterpret_cast<const float*>(R) + (size_t)(mrow + rr * 2) * ldr + ncol);
      }
    }
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) v[rr] = *reinterpret_cast<const f32x4_t*>(my + (rr * 2 + (lane >> 5)) * ERS + (lane & 31) * 16) + bv;
    if (ACT != 0) {
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) v[rr] = gelu4(v[rr]);
    }
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      if (RES != 0) v[rr] += res[rr];
      if (OUT_F32)
        store4(reinterpret_cast<float*>(C) + (size_t)(mrow + rr * 2) * ldc + ncol, v[rr]);
      else
        store4(reinterpret_cast<T16*>(C) + (size_t)(mrow + rr * 2) * ldc + ncol, v[rr]);
    }
  }
}

// ---- tail split (gemm_shared.h; gemm_corr.hip runs the same scheme for the fp16c product) -------------------------------------------
// Second launch of a tail-split product: tile n_full + blockIdx.x = the sum of its S slices in slice order, then the tile's epilogue.
static_assert(BM4 * BN4 == kTailTile, "the slabs of the tail split (gemm_shared.h) hold one tile of gemm_16_nt_256p8");
template <typename T16, bool OUT_F32, int RES, int ACT>
__global__ __launch_bounds__(kTailThreads, 2) void gemm_16_fixup(const float* __restrict__ slabs, int S, int n_full, const float* __restrict__ bias,
                                                        const void* __restrict__ R, int ldr, void* __restrict__ C, int ldc, int M, int N,
                                                        int order) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int q = blockIdx.x >> 2, hh = blockIdx.x & 3;       // one 32-rows-per-wave pass of the epilogue per workgroup
  int tm, tn;
  tile_of(n_full + q, M / BM4, N / BN4, order, tm, tn);
  f32x4_t acc[4][8];
  tail_sum_slabs(slabs, q, S, hh, acc);
  p8_epilogue<T16, OUT_F32, RES, ACT>(acc, smem, tm * BM4, tn * BN4, tm, bias, R, ldr, C, ldc, N, nullptr, nullptr, hh, hh + 1);
}

extern "C" size_t ruart_gemm_16_tail_ws_bytes(int M, int N, int K, int cus) {
  if (M <= 0 || N <= 0 || K <= 0 || M % BM4 || N % BN4 || K % 128) return 0;
  return tail_plan_bytes(tail_plan((M / BM4) * (N / BN4), K / BK, cus, false));
}

// tail_ws / tail_ws_bytes / cus: the slab workspace of ruart_gemm_16_nt_ws and the CU count its plan is made for (NULL: no tail split)
template <typename T16, bool OF, int RS, int AC>
static void launch_one(const T16* a, int lda, const T16* w, int ldw, const float* bias, const void* residual, int ldr, void* C, int ldc,
                       int M, int N, int K, void* tail_ws, size_t tail_ws_bytes, int cus, hipStream_t s) {
  constexpr int lds = 2 * 2 * BM4 * BK * 2;              // 128 KB: both 256x256 kernels
  const bool sq = M % BM4 == 0 && N % BN4 == 0;
  if (g_gemm_variant == 7 && sq && K % BK == 0 && K >= 2 * BK && AC <= 1) {
    auto kern = gemm_16_nt_256w4<T16, OF, RS, AC>;
    static bool done = (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds), true);
    (void)done;
    const int order = g_tile_order_auto ? ruart_tile_group_m(M / BM4, N / BN4, K, false) : g_tile_order;
    hipLaunchKernelGGL(kern, dim3((M / BM4) * (N / BN4)), dim3(256), lds, s, a, lda, w, ldw, bias, residual, ldr, C, ldc, M, N, K, order);
  } else if (g_gemm_variant >= 5 && sq && K % (2 * BK) == 0) {
    auto kern = gemm_16_nt_256p8<T16, OF, RS, AC>;
    static bool done = (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds), true);
    (void)done;
    // GROUP_M from the tile counts (ruart_tile_group_m, gemm_shared.h) until ruart_gemm_set_tile_order pins a value
    const int order = g_tile_order_auto ? ruart_tile_group_m(M / BM4, N / BN4, K, false) : g_tile_order;
    const TailPlan tp = tail_plan_ws((M / BM4) * (N / BN4), K / BK, cus, false, tail_ws, tail_ws_bytes);
    hipLaunchKernelGGL(kern, dim3(tp.n_full + tp.r * tp.S), dim3(512), lds, s, a, lda, w, ldw, bias, residual, ldr, C, ldc, M, N, K,
                       order, 0, (void*)nullptr, (float*)nullptr, tp.n_full, tp.S, (float*)tail_ws, CorrFold{});
    if (tp.r > 0) {
      constexpr int flds = 8 * 32 * 272;
      auto fix = gemm_16_fixup<T16, OF, RS, AC>;
      static bool fdone = (hipFuncSetAttribute((const void*)fix, hipFuncAttributeMaxDynamicSharedMemorySize, flds), true);
      (void)fdone;
      hipLaunchKernelGGL(fix, dim3(4 * tp.r), dim3(512), flds, s, (const float*)tail_ws, tp.S, tp.n_full, bias, residual, ldr, C, ldc, M, N, order);
    }
  } else if (g_gemm_variant >= 3 && sq) {
    auto kern = gemm_16_nt_256sq<T16, OF, RS, AC>;
    static bool done = (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds), true);
    (void)done;
    hipLaunchKernelGGL(kern, dim3((M / BM4) * (N / BN4)), dim3(512), lds, s, a, lda, w, ldw, bias, residual, ldr, C, ldc, M, N, K,
                       g_tile_order);
  } else {
    hipLaunchKernelGGL((gemm_16_nt_128<T16, OF, RS, AC>), dim3((M / BM) * (N / BN)), dim3(256), 0, s, a, lda, w, ldw, bias, residual,
                       ldr, C, ldc, M, N, K, g_tile_order);
  }
}

template <typename T16>
static int launch_gemm16(const void* A, int lda, const void* W, int ldw, const float* bias, const void* residual, int ldr, int res,
                         void* C, int ldc, bool of, int M, int N, int K, int act, void* tail_ws, size_t tail_ws_bytes, int cus,
                         hipStream_t s) {
  const T16* a = (const T16*)A;
  const T16* w = (const T16*)W;
#define LAUNCH(OF, RS, AC) launch_one<T16, OF, RS, AC>(a, lda, w, ldw, bias, residual, ldr, C, ldc, M, N, K, tail_ws, tail_ws_bytes, cus, s)
  if (act == RUART_ACT_GELU) {
    if (res != 0) return (int)hipErrorInvalidValue;
    if (of) LAUNCH(true, 0, 1); else LAUNCH(false, 0, 1);
  } else if (res == 0) {
    if (of) LAUNCH(true, 0, 0); else LAUNCH(false, 0, 0);
  } else if (res == 1) {
    if (of) LAUNCH(true, 1, 0); else LAUNCH(false, 1, 0);
  } else {
    if (of) LAUNCH(true, 2, 0); else LAUNCH(false, 2, 0);
  }
#undef LAUNCH
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_gemm_16_nt_ws(const void* A, int lda, const void* W, int ldw, const float* bias, const void* residual, int ldr,
                                   int residual_dtype, void* C, int ldc, int out_dtype, int M, int N, int K, int act, int in_dtype,
                                   void* tail_ws, size_t tail_ws_bytes, int cus, void* stream) {
  RUART_ENTRY();
  // every argument check sits in front of ruart_prof_begin_: an error return never leaves a profiling event open
  if (M <= 0 || N <= 0 || K <= 0 || M % BM || N % BN || K % BK) return (int)hipErrorInvalidValue;
  if ((lda & 7) || (ldw & 7) || (ldc & 3) || lda < K || ldw < K || ldc < N || !A || !W || !C) return (int)hipErrorInvalidValue;
  if (residual && ((ldr & 3) || ldr < N || act == RUART_ACT_GELU)) return (int)hipErrorInvalidValue;
  if (act != RUART_ACT_NONE && act != RUART_ACT_GELU) return (int)hipErrorInvalidValue;
  if (in_dtype != RUART_DT_BF16 && in_dtype != RUART_DT_F16) return (int)hipErrorInvalidValue;
  if (out_dtype != RUART_DT_F32 && out_dtype != in_dtype) return (int)hipErrorInvalidValue;
  if (residual && residual_dtype != RUART_DT_F32 && residual_dtype != in_dtype) return (int)hipErrorInvalidValue;
  const int res = residual ? (residual_dtype == RUART_DT_F32 ? 2 : 1) : 0;
  const bool of = out_dtype == RUART_DT_F32;
  if (cus <= 0) tail_ws = nullptr;
  void* rec = ruart_prof_begin_((hipStream_t)stream, M, N, K);
  int rc;
  if (in_dtype == RUART_DT_BF16)
    rc = launch_gemm16<bf16_t>(A, lda, W, ldw, bias, residual, ldr, res, C, ldc, of, M, N, K, act, tail_ws, tail_ws_bytes, cus, (hipStream_t)stream);
  else
    rc = launch_gemm16<f16_t>(A, lda, W, ldw, bias, residual, ldr, res, C, ldc, of, M, N, K, act, tail_ws, tail_ws_bytes, cus, (hipStream_t)stream);
  ruart_prof_end_(rec, (hipStream_t)stream);
  return rc;
}

extern "C" int ruart_gemm_16_nt(const void* A, int lda, const void* W, int ldw, const float* bias, const void* residual, int ldr,
                                int residual_dtype, void* C, int ldc, int out_dtype, int M, int N, int K, int act, int in_dtype,
                                void* stream) {
  return ruart_gemm_16_nt_ws(A, lda, W, ldw, bias, residual, ldr, residual_dtype, C, ldc, out_dtype, M, N, K, act, in_dtype, nullptr, 0, 0, stream);
}

// Training forward of the intermediate dense (Models/Bert/modeling.py:287-288): G = gelu(A . W^T + bias) AND the pre-activation H, both in
// the operands' 16-bit type with row stride ldc - the backward pass needs H, the next product needs G, and a separate GELU pass would
// read H back (1.4 ms of the unlocked step).
template <typename T16>
static void launch_gelu2(const void* A, int lda, const void* W, int ldw, const float* bias, void* Hout, void* G, int ldc, int M, int N, int K,
                         hipStream_t s) {
  constexpr int lds = 2 * 2 * BM4 * BK * 2;
  auto kern = gemm_16_nt_256p8<T16, false, 0, 2>;
  static bool done = (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds), true);
  (void)done;
  hipLaunchKernelGGL(kern, dim3((M / BM4) * (N / BN4)), dim3(512), lds, s, (const T16*)A, lda, (const T16*)W, ldw, bias, (const void*)nullptr, 0, G,
                     ldc, M, N, K, g_tile_order, 0, Hout, (float*)nullptr, (M / BM4) * (N / BN4), 0, (float*)nullptr, CorrFold{});
}

extern "C" int ruart_gemm_16_nt_gelu2(const void* A, int lda, const void* W, int ldw, const float* bias, void* H16, void* G16, int ldc, int M,
                                      int N, int K, int in_dtype, void* stream) {
  RUART_ENTRY();
  if (M <= 0 || N <= 0 || K <= 0 || M % BM4 || N % BN4 || K % 128 || (lda & 7) || (ldw & 7) || (ldc & 3) || lda < K || ldw < K || ldc < N || !H16 ||
      !G16 || !A || !W || (in_dtype != RUART_DT_BF16 && in_dtype != RUART_DT_F16))
    return (int)hipErrorInvalidValue;
  void* rec = ruart_prof_begin_((hipStream_t)stream, M, N, K);
  if (in_dtype == RUART_DT_BF16)
    launch_gelu2<bf16_t>(A, lda, W, ldw, bias, H16, G16, ldc, M, N, K, (hipStream_t)stream);
  else
    launch_gelu2<f16_t>(A, lda, W, ldw, bias, H16, G16, ldc, M, N, K, (hipStream_t)stream);
  ruart_prof_end_(rec, (hipStream_t)stream);
  RUART_CHECK_LAUNCH();
  return 0;
}

// Backward of the feed-forward's second half up to the intermediate dense output, in one kernel (Models/Bert/modeling.py:287-288, 300 under
// autograd): acc = dY . W2 (dY (M x K) bf16 gradient at the output dense, Wt = W2^T (N x K) bf16), then per element with the saved f16
// pre-activation H:  dH = acc * gelu'(H)  and  G = gelu(H), both bf16 (M x N); colpart[(M / 128) x N] = column sums of dH per 128-row
// strip before rounding (summed in strip order by the caller: the intermediate bias gradient).  Replaces a GEMM that wrote acc in bf16, an
// elementwise pass that read it back with H (1.1 GB of traffic per layer at the bench shape) and a column-sum pass.
extern "C" size_t ruart_gemm_16_nt_gelu_bwd_ws_floats(int M, int N) { return (size_t)(M / 128) * N; }

extern "C" int ruart_gemm_16_nt_gelu_bwd(const void* dY_bf16, int lda, const void* Wt_bf16, int ldw, const void* H16, int ldh, void* dH_bf16,
                                         void* G_bf16, int ldc, float* colpart, int M, int N, int K, void* stream) {
  RUART_ENTRY();
  if (M <= 0 || N <= 0 || K <= 0 || M % BM4 || N % BN4 || K % 128 || (lda & 7) || (ldw & 7) || (ldc & 3) || (ldh & 3) || lda < K || ldw < K || ldc < N ||
      ldh < N || !dY_bf16 || !Wt_bf16 || !H16 || !dH_bf16 || !G_bf16)
    return (int)hipErrorInvalidValue;
  constexpr int lds = 2 * 2 * BM4 * BK * 2;
  auto kern = gemm_16_nt_256p8<bf16_t, false, 0, 3>;
  static bool done = (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds), true);
  (void)done;
  void* rec = ruart_prof_begin_((hipStream_t)stream, M, N, K);
  hipLaunchKernelGGL(kern, dim3((M / BM4) * (N / BN4)), dim3(512), lds, (hipStream_t)stream, (const bf16_t*)dY_bf16, lda, (const bf16_t*)Wt_bf16, ldw,
                     (const float*)nullptr, H16, ldh, dH_bf16, ldc, M, N, K, g_tile_order, 0, G_bf16, colpart, (M / BM4) * (N / BN4), 0, (float*)nullptr, CorrFold{});
  ruart_prof_end_(rec, (hipStream_t)stream);
  RUART_CHECK_LAUNCH();
  return 0;
}

// Split-K form of the 16-bit NT product: part[z] (M x N fp32, row stride ldc, slabs M * ldc floats apart) = A[:, z*kchunk : ...] .
// W[:, z*kchunk : ...]^T for z < ceil(K / kchunk).  For the encoder's weight gradients dW = dY^T . X (M, N = layer widths, K = token
// rows): a 768 x 768 output is 9 tiles, so the reduction is cut into ~28 slices to fill the 256 CUs.
template <typename T16>
static void launch_splitk(const void* A, int lda, const void* W, int ldw, float* part, int ldc, int M, int N, int K, int kchunk, hipStream_t s) {
  constexpr int lds = 2 * 2 * BM4 * BK * 2;
  auto kern = gemm_16_nt_256p8<T16, true, 0, 0>;
  static bool done = (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds), true);
  (void)done;
  const int nz = (K + kchunk - 1) / kchunk;
  hipLaunchKernelGGL(kern, dim3((M / BM4) * (N / BN4), nz), dim3(512), lds, s, (const T16*)A, lda, (const T16*)W, ldw, (const float*)nullptr,
                     (const void*)nullptr, 0, (void*)part, ldc, M, N, K, g_tile_order, kchunk, (void*)nullptr, (float*)nullptr, (M / BM4) * (N / BN4), 0, (float*)nullptr, CorrFold{});
}

// The projections of the LayerNorm-folded plain 16-bit encoder pass (round 6; CorrFold, gemm_shared.h; the fp16c pass's counterpart is
// ruart_gemm_16c_nt_fold).  kind 0: C (16-bit) = rstd 2^s (A W'^T - mu c) + d (`bias` = d); kind 2: the same, then GELU; kind 3: y = A W^T +
// bias + residual (16-bit rows, normalised with (res_part, res_gamma, res_beta) when res_part != NULL), C = y in 16 bits, out_part[M][4][2]
// = the (sum, sumsq) of the unrounded y per 256-column tile (N <= 1024).  `in_part` NULL with kind 0 / 2 is refused (use ruart_gemm_16_nt).
extern "C" int ruart_gemm_16_nt_fold(const void* A, int lda, const void* W, int ldw, const float* bias, int kind, const float* in_part, int in_np,
                                     const float* colc, float wscale, const void* residual, int ldr, const float* res_part, int res_np,
                                     const float* res_gamma, const float* res_beta, void* C, int ldc, float* out_part, int M, int N, int K,
                                     int stat_len, float eps, int dtype, void* stream) {
  RUART_ENTRY();
  if (M <= 0 || N <= 0 || K <= 0 || M % BM4 || N % BN4 || K % (2 * BK) || (lda & 7) || (ldw & 7) || (ldc & 3) || lda < K || ldw < K || ldc < N)
    return (int)hipErrorInvalidValue;
  if (!A || !W || !C || stat_len <= 0 || (dtype != RUART_DT_F16 && dtype != RUART_DT_BF16)) return (int)hipErrorInvalidValue;
  if (kind == 3) {
    if (!residual || !out_part || N > 256 * kFoldSlots || res_np > kFoldSlots || (res_part && (!res_gamma || !res_beta || res_np <= 0)) || (ldr & 3) ||
        ldr < N)
      return (int)hipErrorInvalidValue;
  } else if (kind == 0 || kind == 2) {
    if (!in_part || !colc || in_np <= 0 || in_np > kFoldSlots) return (int)hipErrorInvalidValue;
  } else {
    return (int)hipErrorInvalidValue;
  }
  hipStream_t s = (hipStream_t)stream;
  CorrFold f{};
  f.in_part = in_part; f.colc = colc; f.in_np = in_np; f.wscale = wscale;
  f.rs_part = res_part; f.rs_g = res_gamma; f.rs_b = res_beta; f.rs_np = res_np;
  f.out_part = out_part; f.inv_h = 1.0f / (float)stat_len; f.eps = eps;
  constexpr int lds = 2 * 2 * BM4 * BK * 2;
  const int order = g_tile_order_auto ? ruart_tile_group_m(M / BM4, N / BN4, K, false) : g_tile_order;
  const int tiles = (M / BM4) * (N / BN4);
  void* rec = ruart_prof_begin_(s, M, N, K);
#define FOLD_LAUNCH(T, RS, AC, FKV)                                                                                                            \
  do {                                                                                                                                       \
    auto kern = gemm_16_nt_256p8<T, false, RS, AC, FKV>;                                                                                     \
    static bool done = (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds), true);                      \
    (void)done;                                                                                                                              \
    hipLaunchKernelGGL(kern, dim3(tiles), dim3(512), lds, s, (const T*)A, lda, (const T*)W, ldw, bias, residual, ldr, C, ldc, M, N, K, order, 0, \
                       (void*)nullptr, (float*)nullptr, tiles, 0, (float*)nullptr, f);                                                       \
  } while (0)
  if (dtype == RUART_DT_F16) {
    if (kind == 3) FOLD_LAUNCH(f16_t, 1, 0, 3);
    else if (kind == 2) FOLD_LAUNCH(f16_t, 0, 1, 1);
    else FOLD_LAUNCH(f16_t, 0, 0, 1);
  } else {
    if (kind == 3) FOLD_LAUNCH(bf16_t, 1, 0, 3);
    else if (kind == 2) FOLD_LAUNCH(bf16_t, 0, 1, 1);
    else FOLD_LAUNCH(bf16_t, 0, 0, 1);
  }
#undef FOLD_LAUNCH
  ruart_prof_end_(rec, s);
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_gemm_16_nt_splitk(const void* A, int lda, const void* W, int ldw, float* part, int ldc, int M, int N, int K, int kchunk,
                                       int in_dtype, void* stream) {
  RUART_ENTRY();
  if (M <= 0 || N <= 0 || K <= 0 || M % BM4 || N % BN4 || K % 128 || kchunk <= 0 || kchunk % 128 || (lda & 7) || (ldw & 7) || (ldc & 3) || lda < K ||
      ldw < K || ldc < N || !A || !W || !part)
    return (int)hipErrorInvalidValue;
  if (in_dtype == RUART_DT_BF16)
    launch_splitk<bf16_t>(A, lda, W, ldw, part, ldc, M, N, K, kchunk, (hipStream_t)stream);
  else if (in_dtype == RUART_DT_F16)
    launch_splitk<f16_t>(A, lda, W, ldw, part, ldc, M, N, K, kchunk, (hipStream_t)stream);
  else
    return (int)hipErrorInvalidValue;
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_gemm_f32_nt(const float* A, int lda, const float* W, int ldw, const float* bias, const float* residual,
                                 int ldr, float* C, int ldc, int M, int N, int K, int act, void* stream) {
  RUART_ENTRY();
  if (M <= 0 || N <= 0 || K <= 0) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(ceil_div(M, FBM) * ceil_div(N, FBN)), block(256);
  const bool vec = (lda % 4 == 0) && (ldw % 4 == 0) && ((((uintptr_t)A) | ((uintptr_t)W)) % 16 == 0);
  if (vec)
    hipLaunchKernelGGL((gemm_f32_nt_64<true>), grid, block, 0, s, A, lda, W, ldw, bias, residual, ldr, C, ldc, M, N, K, act);
  else
    hipLaunchKernelGGL((gemm_f32_nt_64<false>), grid, block, 0, s, A, lda, W, ldw, bias, residual, ldr, C, ldc, M, N, K, act);
  RUART_CHECK_LAUNCH();
  return 0;
}
