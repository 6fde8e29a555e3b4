// Fused masked cross-attention of the SDNet trunk for 385 .. 1024 keys (fp32, exact-fp32 MFMA): ruart_attn_fwd_wide / ruart_attn_bwd_wide.
//
// The operation, the argument lists and the arithmetic are those of sdnet_attention.hip (ruart_attn_fwd_pscale / _bwd_pscale), whose
// kernels keep the whole key / value panel of a batch element in LDS and therefore stop at 384 keys: a 1024-key panel at 80 floats per
// row is 328 KB against 160 KB of LDS.  Here the panels are walked in KEY BLOCKS of 256 rows; only the 16 x L2 score tile stays in LDS
// for the whole kernel (16 x 1026 floats = 66 KB at 1024 keys), beside one key / value block (256 x 80 floats = 82 KB) and the 16 x 64
// query chunk (4 KB): 152 KB at 1024 keys, one workgroup per CU.
//
// Forward, one workgroup (4 waves) per (batch, 16 query rows):
//   scores   per key block: 4 tiles of 16 keys per wave accumulated in registers over the 64-wide chunks of h (the query chunk is
//            staged again for every block: 16 rows, 1/16 of the block's traffic), then written to the score tile in LDS.  The
//            contraction over h runs in the same chunk order as in the 384-key kernels, so a score has the same bits as there.
//   softmax  ONCE over the complete row, after the last block: 16 lanes per row, strided, xor butterfly - the reduction of the 384-key
//            kernels unchanged.  The probabilities are written out anyway, so nothing is rescaled block by block, and -inf - -inf
//            is formed only where the whole row is masked (NaN, as the reference; raises the NaN flag), never inside a dead block.
//   context  per 64 output columns one accumulator per wave that runs through the key blocks in order: one fmaf chain over all keys,
//            as in the 384-key kernels.
// Backward q has the same shape: dP = gO . v^T per value block into LDS, dS over the complete row, grad_a = dS . k through the key
// blocks.  Backward kv works per 16 key rows and has no key limit: tn_product_pf (attn_tiles.h), the 384-key kernels' own.
// Single-query calls (L1 == 1, no activation, no prob_scale): attn1w_*, copies of attn1_* with a 1024-float row.
// Loads are unconditional with clamped addresses and the LDS strides are the conflict-free ones (attn_tiles.h, sdnet_attention.hip's
// head comment).  No atomics on results; every result repeats bit for bit.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   attn_fwd_wide_kernel      117 VGPRs + 16 AGPRs, 106 SGPRs, no scratch; dynamic LDS 16 x 66 + 16 x ldS + 256 x 80 floats:
//                             112,896 bytes at 385 keys (ldS = 418), 151,808 at 1024 (ldS = 1026)
//   attn_bwd_q_wide_kernel    119 VGPRs + 16 AGPRs, 106 SGPRs, no scratch; the same dynamic LDS
//   attn_bwd_kv_wide_kernel   147 VGPRs + 4 AGPRs, 106 SGPRs, no scratch; dynamic LDS 16 x 66 + 64 x 80 floats = 24,704 bytes
//   attn1w_fwd_kernel         44 VGPRs, 54 SGPRs, no scratch; static LDS 4,112 bytes
//   attn1w_bwd_kernel         52 VGPRs, 54 SGPRs, no scratch; static LDS 4,112 bytes
#include "common.h"
#include "ruart_hip.h"
#include "attn_tiles.h"

#define KB 256                 // key rows per block: 16 tiles of 16, 4 per wave
#define NTB 4                  // key tiles per wave and block
#define ATTN_WIDE_MIN_L2 385   // below: ruart_attn_fwd_pscale / _bwd_pscale
#define ATTN_WIDE_MAX_L2 1024

extern int* ruart_nan_flag_ptr;
extern __shared__ __attribute__((aligned(16))) float dsm[];

// S_s[16][ldS] (cols [j0, j0 + nb)) = A . X^T for the rows [j0, j0 + nb) of X (L2 x n, the key or value panel), accumulated over the
// 64-wide chunks of n.  A: 16 rows from i0 of a (L1 x n) matrix, with `aact`; X with `xact`.
__device__ __forceinline__ void block_scores(float* S_s, int ldS, float* a_s, float* kv_s, const float* A, int i0, int L1, const float* X,
                                             int j0, int nb, int L2, int n, Act aact, Act xact) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ntile = nb / 16;
  f32x4_t acc[NTB];
#pragma unroll
  for (int t = 0; t < NTB; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < n; c0 += CH) {
    __syncthreads();
    stage(a_s, LDA_, 16, A, n, i0, L1, c0, n, aact);
    stage(kv_s, LDA_, nb, X, n, j0, L2, c0, n, xact);
    __syncthreads();
    const int kc = min(CH, (n - c0 + 3) & ~3);
#pragma unroll
    for (int t = 0; t < NTB; ++t) {
      const int jt = wave + 4 * t;
      if (jt < ntile) acc[t] = mma16(a_s, LDA_, kv_s + jt * 16 * LDA_, 1, LDA_, kc, acc[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < NTB; ++t) {
    const int jt = wave + 4 * t;
    if (jt < ntile) {
#pragma unroll
      for (int r = 0; r < 4; ++r) S_s[((lane >> 4) * 4 + r) * ldS + j0 + jt * 16 + (lane & 15)] = acc[t][r];
    }
  }
}

// o (this wave's 16 x 16 tile of the 64 output columns from d0) = S_s[16][L2p] . X[:, d0 ..] through the key blocks in order
__device__ __forceinline__ f32x4_t blocks_product(const float* S_s, int ldS, float* kv_s, const float* X, int L2, int L2p, int d0, int n,
                                                  Act xact) {
  const int wave = threadIdx.x >> 6;
  f32x4_t o = {0.f, 0.f, 0.f, 0.f};
  for (int j0 = 0; j0 < L2p; j0 += KB) {
    const int nb = min(KB, L2p - j0);
    __syncthreads();
    stage(kv_s, LDB_, nb, X, n, j0, L2, d0, n, xact);
    __syncthreads();
    o = mma16(S_s + j0, ldS, kv_s + wave * 16, LDB_, 1, nb, o);
  }
  return o;
}

__global__ __launch_bounds__(256) void attn_fwd_wide_kernel(const float* __restrict__ a, const float* __restrict__ k,
                                                            const float* __restrict__ v, const unsigned char* __restrict__ mask,
                                                            float* __restrict__ out, float* __restrict__ probs, int L1, int L2, int h,
                                                            int D3, int* __restrict__ nan_flag, int relu, const float* __restrict__ diag,
                                                            int diag_len, const float* __restrict__ pscale) {
  const int b = blockIdx.y, i0 = blockIdx.x * 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int L2p = (L2 + 15) & ~15, ldS = lds_probs_stride(L2p);
  float* a_s = dsm;                       // [16][LDA_]
  float* S_s = a_s + 16 * LDA_;           // [16][ldS]
  float* kv_s = S_s + 16 * ldS;           // [KB][LDB_]  (keys use stride LDA_, values LDB_)
  const float* ab = a + (size_t)b * L1 * h;
  const float* kb = k + (size_t)b * L2 * h;
  const float* vb = v + (size_t)b * L2 * D3;

  for (int j0 = 0; j0 < L2p; j0 += KB)
    block_scores(S_s, ldS, a_s, kv_s, ab, i0, L1, kb, j0, min(KB, L2p - j0), L2, h, Act{relu, diag, diag_len}, Act{relu, nullptr, 0});
  __syncthreads();
  // ---- masked softmax over the complete row: 16 lanes per row
  {
    const int row = threadIdx.x >> 4, c = threadIdx.x & 15;
    const unsigned char* mb = mask + (size_t)b * L2;
    float* Sr = S_s + row * ldS;
    float mx = -INFINITY;
    for (int j = c; j < L2; j += 16) {
      const float s = mb[j] ? Sr[j] : -INFINITY;
      Sr[j] = s;
      mx = fmaxf(mx, s);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.f;
    for (int j = c; j < L2; j += 16) {
      const float e = expf(Sr[j] - mx);     // all keys masked => -inf - -inf = NaN, as the reference (Layers.py:290 asserts)
      Sr[j] = e;
      sum += e;
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float inv = 1.0f / sum;
    const bool live = (i0 + row) < L1;
    bool bad = false;
    for (int j = c; j < L2p; j += 16) {
      const float p = (j < L2) ? Sr[j] * inv : 0.f;
      // probability dropout: the context uses p * pscale, the saved probabilities stay pre-dropout
      const float ps = (pscale && live && j < L2) ? pscale[((size_t)b * L1 + i0 + row) * L2 + j] : 1.f;
      Sr[j] = live ? p * ps : 0.f;
      bad |= live && !(p == p);
      if (probs && live && j < L2) probs[((size_t)b * L1 + i0 + row) * L2 + j] = p;
    }
    if (bad && nan_flag) atomicOr(nan_flag, 1);
  }
  // ---- context: out[16][D3] = P . v, 64 output columns per pass (one 16-col tile per wave)
  for (int d0 = 0; d0 < D3; d0 += CH) {
    const f32x4_t o = blocks_product(S_s, ldS, kv_s, vb, L2, L2p, d0, D3, no_act());
    const int d = d0 + wave * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + (lane >> 4) * 4 + r;
      if (i < L1 && d < D3) out[((size_t)b * L1 + i) * D3 + d] = o[r];
    }
  }
}

// backward A: per (batch, 16 query rows)
__global__ __launch_bounds__(256) void attn_bwd_q_wide_kernel(const float* __restrict__ k, const float* __restrict__ v,
                                                              const float* __restrict__ probs, const float* __restrict__ gout,
                                                              float* __restrict__ grad_a, float* __restrict__ dS, int L1, int L2, int h,
                                                              int D3, const float* __restrict__ pa, int relu,
                                                              const float* __restrict__ diag, int diag_len,
                                                              float* __restrict__ grad_diag, const float* __restrict__ pscale) {
  const int b = blockIdx.y, i0 = blockIdx.x * 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int L2p = (L2 + 15) & ~15, ldS = lds_probs_stride(L2p);
  float* g_s = dsm;                       // [16][LDA_]   grad_out chunk
  float* S_s = g_s + 16 * LDA_;           // [16][ldS]    dP then dS
  float* kv_s = S_s + 16 * ldS;           // [KB][LDB_]
  const float* kb = k + (size_t)b * L2 * h;
  const float* vb = v + (size_t)b * L2 * D3;
  const float* gb = gout + (size_t)b * L1 * D3;

  for (int j0 = 0; j0 < L2p; j0 += KB)      // dP = gO . v^T
    block_scores(S_s, ldS, g_s, kv_s, gb, i0, L1, vb, j0, min(KB, L2p - j0), L2, D3, no_act(), no_act());
  __syncthreads();
  {                                         // dS = P * (dP - rowsum(dP * P)), the sum over the complete row
    const int row = threadIdx.x >> 4, c = threadIdx.x & 15;
    const bool live = (i0 + row) < L1;
    const float* Pr = probs + ((size_t)b * L1 + (live ? i0 + row : 0)) * L2;
    float* Sr = S_s + row * ldS;
    float dot = 0.f;
    if (pscale && live) {                  // d/dP of (P * pscale) . v
      const float* Mr = pscale + ((size_t)b * L1 + i0 + row) * L2;
      for (int j = c; j < L2; j += 16) Sr[j] *= Mr[j];
    }
    for (int j = c; j < L2; j += 16) dot += Sr[j] * Pr[j];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    for (int j = c; j < L2p; j += 16) {
      float d = 0.f;
      if (live && j < L2) {
        const float p = Pr[j];
        d = p * (Sr[j] - dot);
        dS[((size_t)b * L1 + i0 + row) * L2 + j] = d;
      }
      Sr[j] = d;
    }
  }
  for (int d0 = 0; d0 < h; d0 += CH) {      // grad_a = dS . k
    const f32x4_t o = blocks_product(S_s, ldS, kv_s, kb, L2, L2p, d0, h, Act{relu, nullptr, 0});
    const int d = d0 + wave * 16 + (lane & 15);
    // o = d(loss)/d(a) with a = ReLU(pa) * diag: chain to pa and to diag
    float gd = 0.f;
    const float dsc = (d < h) ? (diag_len == 1 ? diag[0] : (diag_len > 1 ? diag[d] : 1.f)) : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + (lane >> 4) * 4 + r;
      if (i < L1 && d < h) {
        const size_t at = ((size_t)b * L1 + i) * h + d;
        float g = o[r];
        if (pa) {
          const float pv = pa[at];
          gd += g * (relu ? fmaxf(pv, 0.f) : pv);
          g = (relu && pv <= 0.f) ? 0.f : g * dsc;
        }
        grad_a[at] = g;
      }
    }
    if (grad_diag) {      // vector diag only: sum over this tile's 16 rows = the 4 lanes sharing a column; one partial row
      gd += __shfl_xor(gd, 16, 64);     // per workgroup, summed by the caller in a fixed order (no atomics: deterministic)
      gd += __shfl_xor(gd, 32, 64);
      if ((lane >> 4) == 0 && d < h) grad_diag[((size_t)b * gridDim.x + blockIdx.x) * h + d] = gd;
    }
  }
}

// backward B: per (batch, 16 key rows): grad_k = dS^T . a, grad_v = (P o pscale)^T . gO
__global__ __launch_bounds__(256) void attn_bwd_kv_wide_kernel(const float* __restrict__ a, const float* __restrict__ probs,
                                                               const float* __restrict__ dS, const float* __restrict__ gout,
                                                               float* __restrict__ grad_k, float* __restrict__ grad_v, int L1, int L2,
                                                               int h, int D3, const float* __restrict__ pk, int relu,
                                                               const float* __restrict__ diag, int diag_len,
                                                               const float* __restrict__ pscale) {
  const int b = blockIdx.y, j0 = blockIdx.x * 16;
  float* xt_s = dsm;                   // [16][LDA_]
  float* y_s = xt_s + 16 * LDA_;       // [CH][LDB_]
  const size_t pb = (size_t)b * L1 * L2;
  tn_product_pf(dS + pb, L1, L2, j0, a + (size_t)b * L1 * h, h, grad_k + (size_t)b * L2 * h, xt_s, y_s, Act{relu, diag, diag_len},
                (relu && pk) ? pk + (size_t)b * L2 * h : nullptr, nullptr);
  tn_product_pf(probs + pb, L1, L2, j0, gout + (size_t)b * L1 * D3, D3, grad_v + (size_t)b * L2 * D3, xt_s, y_s, no_act(), nullptr,
                pscale ? pscale + pb : nullptr);
}

// ------------------------------------------------------------------------------------------------
// Single-query form (L1 == 1, no activation, no prob_scale): attn1_fwd_kernel / attn1_bwd_kernel of sdnet_attention.hip with a
// 1024-float row (and grad_k / grad_v written through an fmaf from +0: no -0 in a masked key's rows).  One workgroup per batch
// element; the same arithmetic order per output on every run.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn1w_fwd_kernel(const float* __restrict__ a, const float* __restrict__ k,
                                                         const float* __restrict__ v, const unsigned char* __restrict__ mask,
                                                         float* __restrict__ out, float* __restrict__ probs, int L2, int h, int D3,
                                                         int* __restrict__ nan_flag) {
  __shared__ float p_s[ATTN_WIDE_MAX_L2];
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* ab = a + (size_t)b * h;
  const float* kb = k + (size_t)b * L2 * h;
  const float* vb = v + (size_t)b * L2 * D3;
  for (int j0 = wave * 4; j0 < L2; j0 += 16) {         // a wave takes 4 keys at a time: 4 independent coalesced dot products
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int d = lane; d < h; d += 64) {
      const float av = ab[d];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (j0 + u < L2) s[u] = fmaf(av, kb[(size_t)(j0 + u) * h + d], s[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float t = wave_sum(s[u]);
      if (lane == 0 && j0 + u < L2) p_s[j0 + u] = mask[(size_t)b * L2 + j0 + u] ? t : -INFINITY;
    }
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int j = tid; j < L2; j += 256) mx = fmaxf(mx, p_s[j]);
  mx = block_max<4>(mx, red);
  float sum = 0.f;
  for (int j = tid; j < L2; j += 256) {
    const float e = expf(p_s[j] - mx);                  // all keys masked => NaN, as the reference
    p_s[j] = e;
    sum += e;
  }
  sum = block_sum<4>(sum, red);
  __syncthreads();
  const float inv = 1.0f / sum;
  bool bad = false;
  for (int j = tid; j < L2; j += 256) {
    const float p = p_s[j] * inv;
    p_s[j] = p;
    bad |= !(p == p);
    if (probs) probs[(size_t)b * L2 + j] = p;
  }
  if (bad && nan_flag) atomicOr(nan_flag, 1);
  __syncthreads();
  for (int d = tid; d < D3; d += 256) {                 // context: rows of v read coalesced, keys in order, 8 loads in flight
    float o = 0.f;
    int j = 0;
    for (; j + 8 <= L2; j += 8) {
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = vb[(size_t)(j + u) * D3 + d];
#pragma unroll
      for (int u = 0; u < 8; ++u) o = fmaf(p_s[j + u], t[u], o);
    }
    for (; j < L2; ++j) o = fmaf(p_s[j], vb[(size_t)j * D3 + d], o);
    out[(size_t)b * D3 + d] = o;
  }
}

// grad_v[j] = p_j gO, dp_j = gO . v_j, ds = p (dp - sum p dp), grad_a = sum_j ds_j k_j, grad_k[j] = ds_j a
__global__ __launch_bounds__(256) void attn1w_bwd_kernel(const float* __restrict__ a, const float* __restrict__ k,
                                                         const float* __restrict__ v, const float* __restrict__ probs,
                                                         const float* __restrict__ gout, float* __restrict__ grad_a,
                                                         float* __restrict__ grad_k, float* __restrict__ grad_v, int L2, int h, int D3) {
  __shared__ float ds_s[ATTN_WIDE_MAX_L2];
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* ab = a + (size_t)b * h;
  const float* kb = k + (size_t)b * L2 * h;
  const float* vb = v + (size_t)b * L2 * D3;
  const float* gb = gout + (size_t)b * D3;
  const float* pb = probs + (size_t)b * L2;
  for (int j0 = wave * 4; j0 < L2; j0 += 16) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int d = lane; d < D3; d += 64) {
      const float gv = gb[d];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (j0 + u < L2) s[u] = fmaf(gv, vb[(size_t)(j0 + u) * D3 + d], s[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float t = wave_sum(s[u]);
      if (lane == 0 && j0 + u < L2) ds_s[j0 + u] = t;   // dp_j
    }
  }
  __syncthreads();
  float dot = 0.f;
  for (int j = tid; j < L2; j += 256) dot += ds_s[j] * pb[j];
  dot = block_sum<4>(dot, red);
  __syncthreads();
  for (int j = tid; j < L2; j += 256) ds_s[j] = pb[j] * (ds_s[j] - dot);
  __syncthreads();
  for (int d = tid; d < h; d += 256) {
    float g = 0.f;
    int j = 0;
    for (; j + 8 <= L2; j += 8) {
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = kb[(size_t)(j + u) * h + d];
#pragma unroll
      for (int u = 0; u < 8; ++u) g = fmaf(ds_s[j + u], t[u], g);
    }
    for (; j < L2; ++j) g = fmaf(ds_s[j], kb[(size_t)j * h + d], g);
    grad_a[(size_t)b * h + d] = g;
  }
  // one fmaf from +0, as the accumulators of the tiled kernels start: the same product, and a masked key's rows (p = 0) are +0 bits
  // whatever the sign of the other factor
  for (int e = tid; e < L2 * h; e += 256) grad_k[(size_t)b * L2 * h + e] = fmaf(ds_s[e / h], ab[e % h], 0.f);
  for (int e = tid; e < L2 * D3; e += 256) grad_v[(size_t)b * L2 * D3 + e] = fmaf(pb[e / D3], gb[e % D3], 0.f);
}

// ------------------------------------------------------------------------------------------------
static size_t attn_wide_lds_bytes(int L2) {
  const int L2p = (L2 + 15) & ~15;
  const int ldS = ((L2p + 31) / 32) * 32 + 2;
  return sizeof(float) * (size_t)(16 * LDA_ + 16 * ldS + KB * LDB_);
}
static void attn_wide_allow_big_lds() {
  static const bool done = [] {
    const int bytes = (int)attn_wide_lds_bytes(ATTN_WIDE_MAX_L2);
    (void)hipFuncSetAttribute((const void*)attn_fwd_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    (void)hipFuncSetAttribute((const void*)attn_bwd_q_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    return true;
  }();
  (void)done;
}
static bool attn_wide_args_ok(int diag_len, int B, int L1, int L2, int h, int D3) {
  if (B <= 0 || L1 <= 0 || L2 < ATTN_WIDE_MIN_L2 || L2 > ATTN_WIDE_MAX_L2 || h <= 0 || D3 <= 0) return false;
  return diag_len == 0 || diag_len == 1 || diag_len == h;
}

extern "C" int ruart_attn_fwd_wide(const float* a, const float* k, const float* v, const unsigned char* mask, const float* diag,
                                   int diag_len, int relu, const float* prob_scale, float* out, float* probs, int B, int L1, int L2,
                                   int h, int D3, void* stream) {
  RUART_ENTRY();
  if (!attn_wide_args_ok(diag_len, B, L1, L2, h, D3)) return (int)hipErrorInvalidValue;
  if (L1 == 1 && !relu && diag_len == 0 && !prob_scale) {              // single-query form
    hipLaunchKernelGGL(attn1w_fwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a, k, v, mask, out, probs, L2, h, D3,
                       ruart_nan_flag_ptr);
    RUART_CHECK_LAUNCH();
    return 0;
  }
  attn_wide_allow_big_lds();
  hipLaunchKernelGGL(attn_fwd_wide_kernel, dim3(ceil_div(L1, 16), B), dim3(256), attn_wide_lds_bytes(L2), (hipStream_t)stream, a, k, v, mask,
                     out, probs, L1, L2, h, D3, ruart_nan_flag_ptr, relu, diag_len ? diag : nullptr, diag_len, prob_scale);
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_attn_bwd_wide(const float* a, const float* k, const float* v, const float* probs, const float* grad_out,
                                   const float* diag, int diag_len, int relu, const float* prob_scale, float* grad_a, float* grad_k,
                                   float* grad_v, float* grad_diag, float* ds_ws, int B, int L1, int L2, int h, int D3, void* stream) {
  RUART_ENTRY();
  if (!attn_wide_args_ok(diag_len, B, L1, L2, h, D3)) return (int)hipErrorInvalidValue;
  if (L1 == 1 && !relu && diag_len == 0 && !prob_scale) {              // single-query form (ds_ws unused)
    hipLaunchKernelGGL(attn1w_bwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a, k, v, probs, grad_out, grad_a, grad_k, grad_v,
                       L2, h, D3);
    RUART_CHECK_LAUNCH();
    return 0;
  }
  const bool act = relu || diag_len;
  const float* dg = diag_len ? diag : nullptr;
  attn_wide_allow_big_lds();
  hipLaunchKernelGGL(attn_bwd_q_wide_kernel, dim3(ceil_div(L1, 16), B), dim3(256), attn_wide_lds_bytes(L2), (hipStream_t)stream, k, v, probs,
                     grad_out, grad_a, ds_ws, L1, L2, h, D3, act ? a : nullptr, relu, dg, diag_len, (diag_len > 1) ? grad_diag : nullptr,
                     prob_scale);
  RUART_CHECK_LAUNCH();
  hipLaunchKernelGGL(attn_bwd_kv_wide_kernel, dim3(ceil_div(L2, 16), B), dim3(256), sizeof(float) * (16 * LDA_ + CH * LDB_),
                     (hipStream_t)stream, a, probs, ds_ws, grad_out, grad_k, grad_v, L1, L2, h, D3, k, relu, dg, diag_len, prob_scale);
  RUART_CHECK_LAUNCH();
  return 0;
}
