// Row-wise (HBM-bound) kernels of the BERT encoder path.
//
//   ruart_bert_embed_ln      Models/Bert/modeling.py:185-199  word+position+type gather, sum, LayerNorm
//   ruart_rows_layernorm     Models/Bert/modeling.py:164-168  TF-style LN (eps inside sqrt) of the fp32
//                            "dense + bias + residual" rows written by the GEMM epilogue (:263, :302)
//   ruart_bert_attention     Models/Bert/modeling.py:234-250  scores/sqrt(d) + mask, softmax, P.V per head,
//                            variable-length: padded tokens do not exist in the packed stream
//   ruart_bert_pool_mix      Models/Bert/Bert.py:149-165 + Models/SDNet.py:573-581: per-word mean over its
//                            word-piece span of ALL layers, mixed with softmax(alpha)*gamma, in one pass
//   ruart_bert_pool_mix_bwd  gradient of that mix w.r.t. the per-layer weights (alpha/gamma are trainable)
//
// All math is fp32; storage type T of activations is float (validation mode) or bf16.
#include <stdlib.h>
#include "common.h"
#include <type_traits>
#include "ruart_hip.h"

// ---------------------------------------------------------------------------------------------
// one wave per row; lane owns float4 groups at columns (i*64 + lane)*4, i < H/256 (H % 4 == 0, H <= 1024)
// ---------------------------------------------------------------------------------------------
#define MAXG 4

// where a finished row goes: one tensor in the storage type, or the "f16 + fp8 correction" triple of RUART_DT_F16C (fp32 row for
// the residual stream and the pooling kernel, f16 row + the two e4m3 halves for the next GEMM; common.h)
template <typename TOut>
struct RowStorePlain {
  TOut* out;
  __device__ __forceinline__ void operator()(int c, f32x4_t o) const { store4(out + c, o); }
};
struct RowStoreSplit {
  float* o32;
  f16_t* o16;
  unsigned char* o8;
  int H;
  __device__ __forceinline__ void operator()(int c, f32x4_t o) const {
    store4(o32 + c, o);
    store_split4(o16 + c, o8 + c, H, o);
  }
};

template <typename Store>
__device__ __forceinline__ void ln_row_finish(f32x4_t (&v)[MAXG], int H, int lane, const float* gamma, const float* beta,
                                              float eps, const Store& out) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXG; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
  }
  const float mean = wave_sum(s) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXG; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d = v[i][r] - mean;
        q += d * d;
      }
    }
  }
  float var = wave_sum(q) / (float)H;
  // A row far from zero (|mean| > its standard deviation; uniform over the wave): the fp32 row sum is good to ~2^-24 of the SUM, and
  // the mean sits on fp32's grid at |mean|, so every centred value is off by up to an ulp of the mean - at mean 30, std 1 several f16
  // ulps of the outputs near zero.  The centred values are (nearly) exact differences, so their sum recovers what was lost; it stays a
  // separate low part of the mean (mean + mlo would round back onto the same grid), and the second moment is taken again.  Rows whose
  // sums are exact (constant rows) get mlo == 0.  Every other row keeps the plain two-pass arithmetic above, bit for bit.
  // Why a guard and not every row: the compensation moves the last bits of every LayerNorm output of the encoder, and with it on
  // unconditionally tests/test_gpu_dp_global_batch.py (two ranks against one B = 8 step) saw one trunk gradient at 1.08e-4 of its 1e-4
  // bound.  Hidden rows of a real encoder have |mean| well below their std and almost never take this branch: it serves rows with a
  // large offset (tests/test_gpu_encoder_kernels.py), at the price of a discontinuity of ~2^-24 |mean| / std at the threshold, where
  // a row just under it keeps the plain mean.
  float mlo = 0.f;
  if (mean * mean > var) {
    float e = 0.f;
#pragma unroll
    for (int i = 0; i < MAXG; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < H) e += ((v[i][0] - mean) + (v[i][1] - mean)) + ((v[i][2] - mean) + (v[i][3] - mean));
    }
    mlo = wave_sum(e) / (float)H;
    q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXG; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < H) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float d = (v[i][r] - mean) - mlo;
          q += d * d;
        }
      }
    }
    var = wave_sum(q) / (float)H;
  }
  const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
  for (int i = 0; i < MAXG; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
      const f32x4_t g = load4(gamma + c), b = load4(beta + c);
      f32x4_t o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = g[r] * (((v[i][r] - mean) - mlo) * rstd) + b[r];
      out(c, o);
    }
  }
}

template <typename TOut>
__global__ __launch_bounds__(256) void rows_layernorm_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, TOut* __restrict__ out,
                                                             int ldo, int rows, int H) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  f32x4_t v[MAXG];
#pragma unroll
  for (int i = 0; i < MAXG; ++i) {
    const int c = (i * 64 + lane) * 4;
    v[i] = (c < H) ? load4(x + (size_t)row * ldx + c) : (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
  ln_row_finish(v, H, lane, gamma, beta, eps, RowStorePlain<TOut>{out + (size_t)row * ldo});
}

__global__ __launch_bounds__(256) void rows_layernorm_split_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, float eps, float* __restrict__ o32,
                                                                   f16_t* __restrict__ o16, unsigned char* __restrict__ o8, int ldo,
                                                                   int rows, int H) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  f32x4_t v[MAXG];
#pragma unroll
  for (int i = 0; i < MAXG; ++i) {
    const int c = (i * 64 + lane) * 4;
    v[i] = (c < H) ? load4(x + (size_t)row * ldx + c) : (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
  ln_row_finish(v, H, lane, gamma, beta, eps,
                RowStoreSplit{o32 + (size_t)row * ldo, o16 + (size_t)row * ldo, o8 + (size_t)row * 2 * ldo, H});
}

template <typename Store>
__device__ __forceinline__ void embed_ln_row(const int* __restrict__ ids, const int* __restrict__ pos, const float* __restrict__ word,
                                             const float* __restrict__ ptab, const float* __restrict__ type0,
                                             const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int row, int H,
                                             int lane, const Store& out) {
  const size_t wi = (size_t)ids[row] * H, pi = (size_t)pos[row] * H;
  f32x4_t v[MAXG];
#pragma unroll
  for (int i = 0; i < MAXG; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
      // (word + position) + type, in the reference's order (modeling.py:196)
      v[i] = (load4(word + wi + c) + load4(ptab + pi + c)) + load4(type0 + c);
    } else {
      v[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    }
  }
  ln_row_finish(v, H, lane, gamma, beta, eps, out);
}

template <typename TOut>
__global__ __launch_bounds__(256) void embed_ln_kernel(const int* __restrict__ ids, const int* __restrict__ pos,
                                                       const float* __restrict__ word, const float* __restrict__ ptab,
                                                       const float* __restrict__ type0, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float eps, TOut* __restrict__ out, int ldo,
                                                       int rows, int H) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  embed_ln_row(ids, pos, word, ptab, type0, gamma, beta, eps, row, H, lane, RowStorePlain<TOut>{out + (size_t)row * ldo});
}

__global__ __launch_bounds__(256) void embed_ln_split_kernel(const int* __restrict__ ids, const int* __restrict__ pos,
                                                             const float* __restrict__ word, const float* __restrict__ ptab,
                                                             const float* __restrict__ type0, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, float* __restrict__ o32,
                                                             f16_t* __restrict__ o16, unsigned char* __restrict__ o8, int ldo, int rows,
                                                             int H) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  embed_ln_row(ids, pos, word, ptab, type0, gamma, beta, eps, row, H, lane,
               RowStoreSplit{o32 + (size_t)row * ldo, o16 + (size_t)row * ldo, o8 + (size_t)row * 2 * ldo, H});
}

// ---------------------------------------------------------------------------------------------
// Variable-length self-attention, head_dim 64.  One wave per (query block, head); lane = one query token.
// A query block is <= 64 consecutive packed tokens [q0, q1) and a key range [k0, k1) that covers every
// sequence touching the block (host-built, sequence-aligned).  Each lane walks only the keys of ITS
// sequence [tok_lo, tok_hi): trip count = longest sequence in the block, not the block width, so tiny
// OCR items (3-8 word pieces) cost 3-8 iterations.  K/V rows live in LDS, row stride padded by 16 B so
// that lanes reading different rows at the same column hit different banks; lanes of one sequence read
// the same row (broadcast).  Online softmax in registers; Q is pre-scaled by 1/sqrt(64) (folded into
// the Q projection weights, exact in binary).
// ---------------------------------------------------------------------------------------------
template <typename T>
struct KVRow {
  static constexpr int kStride = 64 * (int)sizeof(T) + 16;   // bytes
};

template <typename T, bool SPLIT = false>
__global__ __launch_bounds__(64) void attn_varlen_kernel(const T* __restrict__ qkv, int ld, T* __restrict__ ctx, int ldc, int H,
                                                         const int* __restrict__ bq0, const int* __restrict__ bq1,
                                                         const int* __restrict__ bk0, const int* __restrict__ bk1,
                                                         const int* __restrict__ tok_lo, const int* __restrict__ tok_hi,
                                                         const float* __restrict__ key_bias, f16_t* __restrict__ ctx16 = nullptr,
                                                         unsigned char* __restrict__ ctx8 = nullptr) {
  constexpr int RS = KVRow<T>::kStride;
  __shared__ __attribute__((aligned(16))) char Ks[64 * RS];
  __shared__ __attribute__((aligned(16))) char Vs[64 * RS];
  const int b = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
  const int q0 = bq0[b], q1 = bq1[b], k0 = bk0[b], k1 = bk1[b];
  const int t = q0 + lane;
  const bool active = t < q1;
  float q[64];
  {
    const T* qp = qkv + (size_t)(active ? t : q0) * ld + h * 64;
#pragma unroll
    for (int d = 0; d < 64; d += 4) {
      const f32x4_t v = load4(qp + d);
      q[d] = v[0]; q[d + 1] = v[1]; q[d + 2] = v[2]; q[d + 3] = v[3];
    }
  }
  const int lo = active ? tok_lo[t] : 0, hi = active ? tok_hi[t] : 0;
  float m = -1e30f, l = 0.f;
  float acc[64];
#pragma unroll
  for (int d = 0; d < 64; ++d) acc[d] = 0.f;

  for (int kt = k0; kt < k1; kt += 64) {
    const int tn = min(64, k1 - kt);
    __syncthreads();
    if (lane < tn) {
      const T* kp = qkv + (size_t)(kt + lane) * ld + H + h * 64;
      const T* vp = kp + H;
      constexpr int CH = 16 / (int)sizeof(T);     // elements per 16-byte chunk
#pragma unroll
      for (int c = 0; c < 64 / CH; ++c) {
        *reinterpret_cast<uint4*>(Ks + lane * RS + c * 16) = *reinterpret_cast<const uint4*>(kp + c * CH);
        *reinterpret_cast<uint4*>(Vs + lane * RS + c * 16) = *reinterpret_cast<const uint4*>(vp + c * CH);
      }
    }
    __syncthreads();
    const int jlo = max(lo, kt), jhi = min(hi, kt + tn);
    const int mine = max(0, jhi - jlo);
    int n_it = mine;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_it = max(n_it, __shfl_xor(n_it, o, 64));
    for (int it = 0; it < n_it; ++it) {
      const bool valid = it < mine;
      const int j = valid ? (jlo + it) : kt;
      const T* kr = reinterpret_cast<const T*>(Ks + (j - kt) * RS);
      const T* vr = reinterpret_cast<const T*>(Vs + (j - kt) * RS);
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < 64; d += 4) {
        const f32x4_t kv = load4(kr + d);
        s = fmaf(q[d], kv[0], s); s = fmaf(q[d + 1], kv[1], s); s = fmaf(q[d + 2], kv[2], s); s = fmaf(q[d + 3], kv[3], s);
      }
      if (key_bias) s += key_bias[j];
      const float mn = valid ? fmaxf(m, s) : m;
      const float sc = __expf(m - mn);
      const float p = valid ? __expf(s - mn) : 0.f;
      m = mn;
      l = l * sc + p;
#pragma unroll
      for (int d = 0; d < 64; d += 4) {
        const f32x4_t vv = load4(vr + d);
        acc[d] = fmaf(p, vv[0], acc[d] * sc); acc[d + 1] = fmaf(p, vv[1], acc[d + 1] * sc);
        acc[d + 2] = fmaf(p, vv[2], acc[d + 2] * sc); acc[d + 3] = fmaf(p, vv[3], acc[d + 3] * sc);
      }
    }
  }
  if (active) {
    const float inv = 1.0f / l;
    T* op = ctx + (size_t)t * ldc + h * 64;
#pragma unroll
    for (int d = 0; d < 64; d += 4) {
      const f32x4_t o = {acc[d] * inv, acc[d + 1] * inv, acc[d + 2] * inv, acc[d + 3] * inv};
      if (SPLIT)       // RUART_DT_F16C: the context rows only feed the attention-output GEMM (f16 row + the two e4m3 halves)
        store_split4(ctx16 + (size_t)t * ldc + h * 64 + d, ctx8 + (size_t)t * 2 * ldc + h * 64 + d, H, o);
      else
        store4(op + d, o);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// MFMA flash attention (16-bit modes).  Two kernels with one inner step:
//   attn_flash_kernel       windows of several whole short sequences (<= 64 tokens per block, one key tile, block-diagonal mask:
//                           a key belongs to a query's sequence iff their tok_lo agree; the keys' tok_lo ride along in LDS)
//   attn_flash_long_kernel  blocks of up to 128 queries of one long sequence (the (B, 512) north-star shape): every wave owns two
//                           16-query column blocks, so each K and V^T fragment fetched from LDS feeds two MFMAs; K/V tiles are
//                           double-buffered (the next tile's global loads are in flight under this tile's MFMAs, one barrier per
//                           tile); no per-lane range tests - the ragged last tile is masked through the staged key bias (-1e30)
// Everything is laid out "query on lane&15":
//   S^T (keys x queries) = K . Q^T      A = K rows from LDS (ds_read_b128), B = Q fragments held in registers
//   online softmax per query column: 16 scores per lane + two cross-lane-group shuffles; exp2 with log2(e) folded into one FMA
//   O^T (d x queries)   += V^T . P^T    B = the S^T accumulators themselves (converted to 16-bit, no data movement:
//                                       an accumulator tile is a valid B operand with a permuted k order, cdna guide
//                                       section 3), A = V^T fetched with ds_read_b64_tr_b16 (hardware transpose, T10)
//                                       in the SAME permuted key order: element j of lane group g = key 16(j>>2)+4g+(j&3).
// K/V tiles of 64 keys are staged through registers into LDS rows of 128+16 bytes (conflict-light for both the row
// reads and the transposed reads); rows past the sequence end are zero-filled so masked probabilities never meet NaNs.
// __launch_bounds__(256, 2) keeps the accumulators in architectural VGPRs (the softmax reads them with VALU instructions).
// ---------------------------------------------------------------------------------------------
typedef __attribute__((__vector_size__(4 * sizeof(short)))) short tr16x4_t;
typedef __attribute__((address_space(3))) tr16x4_t* tr_ptr_t;
typedef __attribute__((__vector_size__(4 * sizeof(int)))) int i32x4_t;

__device__ __forceinline__ float max3f(float a, float b, float c) {       // no NaN-quieting copies: inputs are never NaN here
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// One online-softmax step of a 16-query column block over a 64-key tile: sacc (scores, masked entries = -1e30) -> probabilities
// as the two 16-bit B fragments of the P.V product; running max m, sum l and the output accumulators are updated.
template <typename T16>
__device__ __forceinline__ void flash_softmax_step(f32x4_t (&sacc)[4], float& m, float& l, f32x4_t (&o)[4],
                                                   typename Vec8<T16>::type (&pf)[2]) {
  constexpr float kLog2e = 1.4426950408889634f;
  float mx = max3f(sacc[0][0], sacc[0][1], sacc[0][2]);
  mx = max3f(mx, sacc[0][3], sacc[1][0]);
  mx = max3f(mx, sacc[1][1], sacc[1][2]);
  mx = max3f(mx, sacc[1][3], sacc[2][0]);
  mx = max3f(mx, sacc[2][1], sacc[2][2]);
  mx = max3f(mx, sacc[2][3], sacc[3][0]);
  mx = max3f(mx, sacc[3][1], sacc[3][2]);
  mx = max3f(mx, sacc[3][3], m);
  mx = max3f(mx, __shfl_xor(mx, 16, 64), m);
  const float mn = max3f(mx, __shfl_xor(mx, 32, 64), m);
  const float mn2 = mn * kLog2e;
  float rs = 0.f;
#pragma unroll
  for (int it = 0; it < 4; ++it)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[it][r], kLog2e, -mn2));
      sacc[it][r] = p;
      rs += p;
    }
  rs += __shfl_xor(rs, 16, 64);
  rs += __shfl_xor(rs, 32, 64);
  if (__any(mn > m)) {                                   // the running maximum rarely moves after the first tiles
    const float scl = __builtin_amdgcn_exp2f(m * kLog2e - mn2);
    l *= scl;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] *= scl;
    m = mn;
  }
  l += rs;
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pf[s2][j] = (T16)sacc[2 * s2][j];
      pf[s2][4 + j] = (T16)sacc[2 * s2 + 1][j];
    }
}

// Workgroup -> (block, head) for the MFMA attention kernels: a 1-D grid, every XCD takes a contiguous
// chunk of the logical ids (xcd_remap) and inside it the HEAD index runs fastest (short windows: the 12 x 256-byte slices of a token
// row are fetched by neighbouring workgroups at the same time instead of by workgroups ~700 launches apart) or, for the long-sequence
// kernel, the query blocks of one (sequence, head) are neighbours on ONE XCD (they all stream the same K / V rows: the second to
// fourth reader hits that XCD's L2 instead of the fabric).
#define ATTN_QGROUP 4
__device__ __forceinline__ void attn_block_head(int n_heads, bool long_blocks, int n_blocks, int& b, int& h) {
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  if (!long_blocks) {
    b = id / n_heads;
    h = id - b * n_heads;
  } else {                     // groups of ATTN_QGROUP consecutive query blocks (one 512-token sequence = 4 blocks of 128) x heads
    const int per = ATTN_QGROUP * n_heads;
    const int g = id / per, first = g * ATTN_QGROUP;
    const int gsz = min(ATTN_QGROUP, n_blocks - first);
    const int r = id - g * per;
    h = r / gsz;
    b = first + (r - h * gsz);
  }
}
static inline dim3 attn_grid(int n_blocks, int n_heads) {
  return dim3((unsigned)n_blocks * (unsigned)n_heads);
}

template <typename T16>
__global__ __launch_bounds__(256, 2) void attn_flash_kernel(const T16* __restrict__ qkv, int ld, T16* __restrict__ ctx, int ldc, int H,
                                                            const int* __restrict__ bq0, const int* __restrict__ bq1,
                                                            const int* __restrict__ bk0, const int* __restrict__ bk1,
                                                            const int* __restrict__ tok_lo, const float* __restrict__ key_bias) {
  constexpr int RS = 144;
  __shared__ __attribute__((aligned(16))) char Ks[64 * RS];
  __shared__ __attribute__((aligned(16))) char Vs[64 * RS];
  __shared__ __attribute__((aligned(16))) float Bs[64];
  __shared__ __attribute__((aligned(16))) int Ls[64];
  typedef typename Vec8<T16>::type frag_t;
  int b, h;
  attn_block_head(H >> 6, false, 0, b, h);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int q0 = bq0[b], q1 = bq1[b], k0 = bk0[b], k1 = bk1[b];
  const int tq = q0 + wave * 16 + fr;
  const bool qvalid = tq < q1;
  // a query attends to the keys of its own sequence = the keys whose first-token index equals its own; lanes past the block's
  // last query shadow query q0 (real scores, nothing stored)
  const int lo = tok_lo[qvalid ? tq : q0];

  frag_t qf[2];
  {
    const T16* qp = qkv + (size_t)(qvalid ? tq : q0) * ld + h * 64 + g * 8;
    qf[0] = *reinterpret_cast<const frag_t*>(qp);
    qf[1] = *reinterpret_cast<const frag_t*>(qp + 32);
  }
  float m = -1e30f, l = 0.f;
  f32x4_t o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int srow = tid >> 2, sc0 = (tid & 3) * 2;       // staging: row 0..63, two 16-byte chunks
  for (int kt = k0; kt < k1; kt += 64) {
    const int tn = min(64, k1 - kt);
    __syncthreads();
    {
      uint4 kv[2], vv[2];
      if (srow < tn) {
        const T16* kp = qkv + (size_t)(kt + srow) * ld + H + h * 64 + sc0 * 8;
        kv[0] = *reinterpret_cast<const uint4*>(kp);
        kv[1] = *reinterpret_cast<const uint4*>(kp + 8);
        vv[0] = *reinterpret_cast<const uint4*>(kp + H);
        vv[1] = *reinterpret_cast<const uint4*>(kp + H + 8);
      } else {
        kv[0] = kv[1] = vv[0] = vv[1] = make_uint4(0, 0, 0, 0);
      }
      *reinterpret_cast<uint4*>(Ks + srow * RS + sc0 * 16) = kv[0];
      *reinterpret_cast<uint4*>(Ks + srow * RS + sc0 * 16 + 16) = kv[1];
      *reinterpret_cast<uint4*>(Vs + srow * RS + sc0 * 16) = vv[0];
      *reinterpret_cast<uint4*>(Vs + srow * RS + sc0 * 16 + 16) = vv[1];
      if (tid < 64) {
        const bool in = tid < tn;
        Ls[tid] = in ? tok_lo[kt + tid] : -1;
        Bs[tid] = (in && key_bias) ? key_bias[kt + tid] : 0.f;
      }
    }
    __syncthreads();

    f32x4_t sacc[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      sacc[it] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const frag_t kf = *reinterpret_cast<const frag_t*>(Ks + (it * 16 + fr) * RS + (ks * 32 + g * 8) * 2);
        sacc[it] = mfma_16x16x32(kf, qf[ks], sacc[it]);
      }
    }
    // sacc[it][r] = score(key kt + it*16 + g*4 + r, query fr)
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const i32x4_t lk = *reinterpret_cast<const i32x4_t*>(&Ls[it * 16 + g * 4]);
      if (key_bias) sacc[it] += *reinterpret_cast<const f32x4_t*>(&Bs[it * 16 + g * 4]);
#pragma unroll
      for (int r = 0; r < 4; ++r) sacc[it][r] = lk[r] == lo ? sacc[it][r] : -1e30f;
    }
    frag_t pf[2];
    flash_softmax_step<T16>(sacc, m, l, o, pf);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        // transposed fetch of V: block rows (keys) 32*s2 + 4g .. +3 and +16, columns dt*16 .. +15; lane 4q+p of the 16-lane
        // group supplies row q, columns 4p..4p+3 and receives column (lane&15), rows 0..3
        const char* base = Vs + (32 * s2 + 4 * g + (fr >> 2)) * RS + (dt * 16 + (fr & 3) * 4) * 2;
        union { struct { tr16x4_t a, b; } s; frag_t f; } u;
        u.s.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)base);
        u.s.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(base + 16 * RS));
        o[dt] = mfma_16x16x32(u.f, pf[s2], o[dt]);
      }
  }
  if (qvalid) {
    const float inv = 1.0f / l;
    T16* op = ctx + (size_t)tq * ldc + h * 64 + g * 4;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) store4(op + dt * 16, o[dt] * inv);
  }
}

// ---------------------------------------------------------------------------------------------
// attn_flash_kernel for the RUART_DT_F16C mode: fp32 [Q | K | V] rows in, context rows out in the split form (f16 + two e4m3
// halves, common.h).  Same structure - windows of whole short sequences or 64-query blocks of a long one, S^T = K . Q^T and
// O^T += V^T . P^T on v_mfma_f32_16x16x32_f16 - but every operand is split into f16 hi + f16 lo on the way to LDS / registers
// and every product is taken as hi.hi + hi.lo + lo.hi (22 significant bits: fp32-class scores and contexts).  Attention is
// ~0.1 % of the encoder's flops at item lengths of 3-8 pieces, so the 3x MFMA count is free; the kernel is bound by its HBM
// bytes (9 KB in, 3 KB out per word piece and layer).
// ---------------------------------------------------------------------------------------------
// hi = f16(x), lo = f16(x - hi) for two values at a time: one v_cvt_pk_f16_f32 and two v_fma_mix{lo,hi}_f16 (x * 1.0 - hi with the f16
// operand read straight from the packed register: the difference is exact in fp32, so the single rounding to f16 is the one the C++
// form (f16)(x - (float)hi) makes - same bits, 1.5 instead of 3.25 VALU instructions per element (hipcc converts every element twice
// and back for that form).  Round 5: these kernels are bound by their VALU issue slots once the loads are out of the way (section 5 (4)).
__device__ __forceinline__ void split2_f16(float x0, float x1, unsigned& hi2, unsigned& lo2) {
  typedef f16_t f16x2v __attribute__((ext_vector_type(2)));
  const f16x2v h = {(f16_t)x0, (f16_t)x1};
  hi2 = __builtin_bit_cast(unsigned, h);
  unsigned r;
  asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(r) : "v"(x0), "v"(hi2));
  asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(r) : "v"(x1), "v"(hi2));
  lo2 = r;
}
__device__ __forceinline__ void split_f16x4(const f32x4_t a, f16x4_t& hi, f16x4_t& lo) {
  union { f16x4_t v; unsigned u[2]; } h, l;
  split2_f16(a[0], a[1], h.u[0], l.u[0]);
  split2_f16(a[2], a[3], h.u[1], l.u[1]);
  hi = h.v;
  lo = l.v;
}
__device__ __forceinline__ void split_f16x8(const f32x4_t a, const f32x4_t b, f16x8_t& hi, f16x8_t& lo) {
  union { f16x8_t v; unsigned u[4]; } h, l;
  split2_f16(a[0], a[1], h.u[0], l.u[0]);
  split2_f16(a[2], a[3], h.u[1], l.u[1]);
  split2_f16(b[0], b[1], h.u[2], l.u[2]);
  split2_f16(b[2], b[3], h.u[3], l.u[3]);
  hi = h.v;
  lo = l.v;
}
// lo half of an already rounded pair: lo2 = f16x2(x0 - hi2.lo, x1 - hi2.hi)
__device__ __forceinline__ unsigned lo2_of(float x0, float x1, unsigned hi2) {
  unsigned r;
  asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(r) : "v"(x0), "v"(hi2));
  asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(r) : "v"(x1), "v"(hi2));
  return r;
}

#define ATTN_LD4(p) load4_stream(p)          // the fp32 Q / K / V rows are read once per layer (common.h)
__global__ __launch_bounds__(256, 2) void attn_flash_split_kernel(const float* __restrict__ qkv, int ld, f16_t* __restrict__ ctx16,
                                                                  unsigned char* __restrict__ ctx8, int ldc, int H,
                                                                  const int* __restrict__ bq0, const int* __restrict__ bq1,
                                                                  const int* __restrict__ bk0, const int* __restrict__ bk1,
                                                                  const int* __restrict__ tok_lo, const float* __restrict__ key_bias) {
  constexpr int RS = 144;
  __shared__ __attribute__((aligned(16))) char Kh[64 * RS];
  __shared__ __attribute__((aligned(16))) char Kl[64 * RS];
  __shared__ __attribute__((aligned(16))) char Vh[64 * RS];
  __shared__ __attribute__((aligned(16))) char Vl[64 * RS];
  __shared__ __attribute__((aligned(16))) float Bs[64];
  __shared__ __attribute__((aligned(16))) int Ls[64];
  typedef f16x8_t frag_t;
  int b, h;
  attn_block_head(H >> 6, false, 0, b, h);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int q0 = bq0[b], q1 = bq1[b], k0 = bk0[b], k1 = bk1[b];
  const int tq = q0 + wave * 16 + fr;
  const bool qvalid = tq < q1;
  const int lo_tok = tok_lo[qvalid ? tq : q0];

  // staging K and V: lane -> (row 16 wave + 4 i + lane / 16, 16-byte piece lane % 16): one load instruction covers four whole
  // 256-byte row slices (8 cache lines, every byte used) where the first form - a lane taking 64 contiguous bytes in four
  // loads - touched 32 lines per instruction, four times over.  The loads of a key tile are issued BEFORE anything waits: the
  // first tile's ahead of the query rows' split (a window of <= 64 tokens has one tile: its whole input is then in flight at
  // once instead of in two dependent round trips), a later tile's ahead of the barrier that frees the LDS images.
  const int prow = lane >> 4, piece = lane & 15;
  f32x4_t kx[4], vx[4];
  int ls_v = -1;
  float bs_v = 0.f;
  auto load_kv = [&](int kt, int tn) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = wave * 16 + i * 4 + prow;
      const float* kp = qkv + (size_t)(kt + min(row, tn - 1)) * ld + H + h * 64 + piece * 4;      // unconditional (clamped) loads
      kx[i] = ATTN_LD4(kp);
      vx[i] = ATTN_LD4(kp + H);
    }
    if (tid < 64) {
      const bool in = tid < tn;
      ls_v = in ? tok_lo[kt + tid] : -1;
      bs_v = (in && key_bias) ? key_bias[kt + tid] : 0.f;
    }
  };
  f32x4_t qx[4];
  {
    const float* qp = qkv + (size_t)(qvalid ? tq : q0) * ld + h * 64 + g * 8;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qx[2 * ks] = ATTN_LD4(qp + ks * 32);
      qx[2 * ks + 1] = ATTN_LD4(qp + ks * 32 + 4);
    }
  }
  load_kv(k0, min(64, k1 - k0));
  frag_t qh[2], ql[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) split_f16x8(qx[2 * ks], qx[2 * ks + 1], qh[ks], ql[ks]);
  float m = -1e30f, l = 0.f;
  f32x4_t o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  for (int kt = k0; kt < k1; kt += 64) {
    const int tn = min(64, k1 - kt);
    if (kt != k0) {
      load_kv(kt, tn);
      __syncthreads();                  // every wave is done reading the previous tile's images
    }
    {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = wave * 16 + i * 4 + prow;
        // (rows past the window are clamped copies of its last row - finite - and their keys are masked through Ls = -1: their
        //  probabilities are exactly 0, so they need no zero-fill; 32 selects per thread and step less)
        f16x4_t kh4, kl4, vh4, vl4;
        split_f16x4(kx[i], kh4, kl4);
        split_f16x4(vx[i], vh4, vl4);
        const int off = row * RS + piece * 8;
        *reinterpret_cast<f16x4_t*>(Kh + off) = kh4;
        *reinterpret_cast<f16x4_t*>(Kl + off) = kl4;
        *reinterpret_cast<f16x4_t*>(Vh + off) = vh4;
        *reinterpret_cast<f16x4_t*>(Vl + off) = vl4;
      }
      if (tid < 64) {
        Ls[tid] = ls_v;
        Bs[tid] = bs_v;
      }
    }
    __syncthreads();

    f32x4_t sacc[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      sacc[it] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int off = (it * 16 + fr) * RS + (ks * 32 + g * 8) * 2;
        const frag_t kfh = *reinterpret_cast<const frag_t*>(Kh + off);
        const frag_t kfl = *reinterpret_cast<const frag_t*>(Kl + off);
        sacc[it] = mfma_16x16x32(kfl, qh[ks], sacc[it]);        // small terms first
        sacc[it] = mfma_16x16x32(kfh, ql[ks], sacc[it]);
        sacc[it] = mfma_16x16x32(kfh, qh[ks], sacc[it]);
      }
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const i32x4_t lk = *reinterpret_cast<const i32x4_t*>(&Ls[it * 16 + g * 4]);
      if (key_bias) sacc[it] += *reinterpret_cast<const f32x4_t*>(&Bs[it * 16 + g * 4]);
#pragma unroll
      for (int r = 0; r < 4; ++r) sacc[it][r] = lk[r] == lo_tok ? sacc[it][r] : -1e30f;
    }
    frag_t ph[2];
    flash_softmax_step<f16_t>(sacc, m, l, o, ph);             // sacc now holds the fp32 probabilities, ph their f16 roundings
    frag_t pl[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      union { frag_t v; unsigned u[4]; } hh, ll;
      hh.v = ph[s2];
      ll.u[0] = lo2_of(sacc[2 * s2][0], sacc[2 * s2][1], hh.u[0]);
      ll.u[1] = lo2_of(sacc[2 * s2][2], sacc[2 * s2][3], hh.u[1]);
      ll.u[2] = lo2_of(sacc[2 * s2 + 1][0], sacc[2 * s2 + 1][1], hh.u[2]);
      ll.u[3] = lo2_of(sacc[2 * s2 + 1][2], sacc[2 * s2 + 1][3], hh.u[3]);
      pl[s2] = ll.v;
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const int off = (32 * s2 + 4 * g + (fr >> 2)) * RS + (dt * 16 + (fr & 3) * 4) * 2;
        union { struct { tr16x4_t a, b; } s; frag_t f; } uh, ul;
        uh.s.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(Vh + off));
        uh.s.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(Vh + off + 16 * RS));
        ul.s.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(Vl + off));
        ul.s.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(Vl + off + 16 * RS));
        o[dt] = mfma_16x16x32(ul.f, ph[s2], o[dt]);
        o[dt] = mfma_16x16x32(uh.f, pl[s2], o[dt]);
        o[dt] = mfma_16x16x32(uh.f, ph[s2], o[dt]);
      }
  }
  if (qvalid) {
    const float inv = 1.0f / l;
    const size_t col = (size_t)h * 64 + g * 4;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      store_split4(ctx16 + (size_t)tq * ldc + col + dt * 16, ctx8 + (size_t)tq * 2 * ldc + col + dt * 16, H, o[dt] * inv);
  }
}

// ---------------------------------------------------------------------------------------------
// attn_flash_split_kernel, several heads per workgroup (round 5).  One window of <= 64 queries per workgroup as before, but the
// workgroup walks HPG consecutive heads (x the window's key tiles) and the global loads of step j + 1 - the next head's K / V
// slices, and its Q rows once the score products of step j have consumed the current ones - are issued as soon as step j's
// operands have left their registers for LDS: they are in flight under step j's MFMAs, softmax and stores.  The one-head kernel
// runs load -> split -> LDS -> MFMA -> store strictly one after the other inside a workgroup and relies on the four workgroups
// of a CU to overlap them (47 % of the HBM rate, waves at issue 55 % of their cycles: profiles/r04_pmc_per_kernel.csv).
// A head's context rows are converted when its last tile is done and WRITTEN one step later, just before that step issues its own
// prefetch: gfx9 counts loads and stores in one in-order vmcnt queue, so stores issued at the end of a step would be drained by the
// next step's first wait for its operands (2-3 us per step, measured with s_memrealtime stamps); issued ahead of the prefetch they
// have a whole step to complete.
// The arithmetic of a (window, head) is the one-head kernel's, instruction for instruction: the outputs are bit-identical.
// ---------------------------------------------------------------------------------------------
template <int HPG>
__global__ __launch_bounds__(256, 2) void attn_flash_split_mh_kernel(const float* __restrict__ qkv, int ld, f16_t* __restrict__ ctx16,
                                                                     unsigned char* __restrict__ ctx8, int ldc, int H,
                                                                     const int* __restrict__ bq0, const int* __restrict__ bq1,
                                                                     const int* __restrict__ bk0, const int* __restrict__ bk1,
                                                                     const int* __restrict__ tok_lo, const float* __restrict__ key_bias) {
  constexpr int RS = 144;
  __shared__ __attribute__((aligned(16))) char Kh[64 * RS];
  __shared__ __attribute__((aligned(16))) char Kl[64 * RS];
  __shared__ __attribute__((aligned(16))) char Vh[64 * RS];
  __shared__ __attribute__((aligned(16))) char Vl[64 * RS];
  __shared__ __attribute__((aligned(16))) float Bs[64];
  __shared__ __attribute__((aligned(16))) int Ls[64];
  typedef f16x8_t frag_t;
  const int n_groups = (H >> 6) / HPG;
  const int id = xcd_remap(blockIdx.x, gridDim.x);          // XCD-contiguous ids, the head GROUP fastest (neighbours share token rows)
  const int b = id / n_groups, h0 = (id - b * n_groups) * HPG;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int q0 = bq0[b], q1 = bq1[b], k0 = bk0[b], k1 = bk1[b];
  const int tq = q0 + wave * 16 + fr;
  const bool qvalid = tq < q1;
  const int lo_tok = tok_lo[qvalid ? tq : q0];
  const int prow = lane >> 4, piece = lane & 15;
  const int n_tiles = (k1 - k0 + 63) >> 6, n_steps = n_tiles * HPG;

  f32x4_t kx[4], vx[4], qx[4];
  int ls_v = -1;
  float bs_v = 0.f;
  auto load_kv = [&](int h, int kt, int tn) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = wave * 16 + i * 4 + prow;
      const float* kp = qkv + (size_t)(kt + min(row, tn - 1)) * ld + H + h * 64 + piece * 4;      // unconditional (clamped) loads
      kx[i] = ATTN_LD4(kp);
      vx[i] = ATTN_LD4(kp + H);
    }
    if (tid < 64) {
      const bool in = tid < tn;
      ls_v = in ? tok_lo[kt + tid] : -1;
      bs_v = (in && key_bias) ? key_bias[kt + tid] : 0.f;
    }
  };
  auto load_q = [&](int h) {
    const float* qp = qkv + (size_t)(qvalid ? tq : q0) * ld + h * 64 + g * 8;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qx[2 * ks] = ATTN_LD4(qp + ks * 32);
      qx[2 * ks + 1] = ATTN_LD4(qp + ks * 32 + 4);
    }
  };
  load_q(h0);
  load_kv(h0, k0, min(64, k1 - k0));
  frag_t qh[2], ql[2];
  float m = -1e30f, l = 0.f;
  f32x4_t o[4];

  // a finished head's context rows in their stored form (f16 x 4, e4m3 lo x 4, e4m3 hi x 4 per 16-column group), written one step later
  f16x4_t pend16[4];
  unsigned pend_lo[4], pend_hi[4];
  int pend_h = -1;
  auto flush_pending = [&]() {
    if (pend_h >= 0 && qvalid) {
      const size_t col = (size_t)pend_h * 64 + g * 4;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        *reinterpret_cast<f16x4_t*>(ctx16 + (size_t)tq * ldc + col + dt * 16) = pend16[dt];
        unsigned char* p8 = ctx8 + (size_t)tq * 2 * ldc + col + dt * 16;
        *reinterpret_cast<unsigned*>(p8) = pend_lo[dt];
        *reinterpret_cast<unsigned*>(p8 + H) = pend_hi[dt];
      }
    }
    pend_h = -1;
  };
  int hh = 0, t = 0;                       // head within the group, key tile within the window
  for (int j = 0; j < n_steps; ++j) {
    const int h = h0 + hh, kt = k0 + t * 64;
    const int tn = min(64, k1 - kt);
    const bool last_tile = t == n_tiles - 1;
    if (t == 0) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) split_f16x8(qx[2 * ks], qx[2 * ks + 1], qh[ks], ql[ks]);
      m = -1e30f;
      l = 0.f;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    }
    {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = wave * 16 + i * 4 + prow;
        // (rows past the window are clamped copies of its last row - finite - and their keys are masked through Ls = -1: their
        //  probabilities are exactly 0, so they need no zero-fill; 32 selects per thread and step less)
        f16x4_t kh4, kl4, vh4, vl4;
        split_f16x4(kx[i], kh4, kl4);
        split_f16x4(vx[i], vh4, vl4);
        const int off = row * RS + piece * 8;
        *reinterpret_cast<f16x4_t*>(Kh + off) = kh4;
        *reinterpret_cast<f16x4_t*>(Kl + off) = kl4;
        *reinterpret_cast<f16x4_t*>(Vh + off) = vh4;
        *reinterpret_cast<f16x4_t*>(Vl + off) = vl4;
      }
      if (tid < 64) {
        Ls[tid] = ls_v;
        Bs[tid] = bs_v;
      }
    }
    flush_pending();                      // the previous head's rows: ahead of the prefetch in the vmcnt queue
    // the next step's K / V slices: in flight from here on (the registers they land in are free)
    const int t_n = last_tile ? 0 : t + 1, hh_n = last_tile ? hh + 1 : hh;
    if (j + 1 < n_steps) {
      load_kv(h0 + hh_n, k0 + t_n * 64, min(64, k1 - (k0 + t_n * 64)));
      if (last_tile) load_q(h + 1);       // the next head's Q rows too (qx is free since this head's split)
    }
    __syncthreads();

    f32x4_t sacc[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      sacc[it] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int off = (it * 16 + fr) * RS + (ks * 32 + g * 8) * 2;
        const frag_t kfh = *reinterpret_cast<const frag_t*>(Kh + off);
        const frag_t kfl = *reinterpret_cast<const frag_t*>(Kl + off);
        sacc[it] = mfma_16x16x32(kfl, qh[ks], sacc[it]);        // small terms first
        sacc[it] = mfma_16x16x32(kfh, ql[ks], sacc[it]);
        sacc[it] = mfma_16x16x32(kfh, qh[ks], sacc[it]);
      }
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const i32x4_t lk = *reinterpret_cast<const i32x4_t*>(&Ls[it * 16 + g * 4]);
      if (key_bias) sacc[it] += *reinterpret_cast<const f32x4_t*>(&Bs[it * 16 + g * 4]);
#pragma unroll
      for (int r = 0; r < 4; ++r) sacc[it][r] = lk[r] == lo_tok ? sacc[it][r] : -1e30f;
    }
    frag_t ph[2];
    flash_softmax_step<f16_t>(sacc, m, l, o, ph);             // sacc now holds the fp32 probabilities, ph their f16 roundings
    frag_t pl[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      union { frag_t v; unsigned u[4]; } hh, ll;
      hh.v = ph[s2];
      ll.u[0] = lo2_of(sacc[2 * s2][0], sacc[2 * s2][1], hh.u[0]);
      ll.u[1] = lo2_of(sacc[2 * s2][2], sacc[2 * s2][3], hh.u[1]);
      ll.u[2] = lo2_of(sacc[2 * s2 + 1][0], sacc[2 * s2 + 1][1], hh.u[2]);
      ll.u[3] = lo2_of(sacc[2 * s2 + 1][2], sacc[2 * s2 + 1][3], hh.u[3]);
      pl[s2] = ll.v;
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const int off = (32 * s2 + 4 * g + (fr >> 2)) * RS + (dt * 16 + (fr & 3) * 4) * 2;
        union { struct { tr16x4_t a, b; } s; frag_t f; } uh, ul;
        uh.s.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(Vh + off));
        uh.s.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(Vh + off + 16 * RS));
        ul.s.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(Vl + off));
        ul.s.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(Vl + off + 16 * RS));
        o[dt] = mfma_16x16x32(ul.f, ph[s2], o[dt]);
        o[dt] = mfma_16x16x32(uh.f, pl[s2], o[dt]);
        o[dt] = mfma_16x16x32(uh.f, ph[s2], o[dt]);
      }
    if (last_tile) {                      // (uniform) convert now, write at the next step
      const float inv = 1.0f / l;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const f32x4_t v = o[dt] * inv;
        const f16x4_t hv = {(f16_t)v[0], (f16_t)v[1], (f16_t)v[2], (f16_t)v[3]};
        pend16[dt] = hv;
        const f32x4_t lo = {v[0] - (float)hv[0], v[1] - (float)hv[1], v[2] - (float)hv[2], v[3] - (float)hv[3]};
        pend_lo[dt] = pack_fp8x4(lo, (float)(1 << RUART_C8_SA_LO));
        pend_hi[dt] = pack_fp8x4(v, (float)(1 << RUART_C8_SA_HI));
      }
      pend_h = h;
    }
    __syncthreads();                      // every wave is done reading this step's images
    t = t_n;
    hh = hh_n;
  }
  flush_pending();
}

// RUART_ATTN_LONG_WPS: minimum waves per SIMD the register allocator has to leave room for (2: 145 VGPRs, three workgroups per CU;
// 4: 128 VGPRs with five spilled, four workgroups per CU)
#define RUART_ATTN_LONG_WPS 2
template <typename T16>
__global__ __launch_bounds__(256, RUART_ATTN_LONG_WPS) void attn_flash_long_kernel(const T16* __restrict__ qkv, int ld, T16* __restrict__ ctx, int ldc, int H,
                                                                 const int* __restrict__ bq0, const int* __restrict__ bq1,
                                                                 const int* __restrict__ bk0, const int* __restrict__ bk1,
                                                                 const float* __restrict__ key_bias, int n_long) {
  constexpr int RS = 144;
  __shared__ __attribute__((aligned(16))) char Ks[2][64 * RS];
  __shared__ __attribute__((aligned(16))) char Vs[2][64 * RS];
  __shared__ __attribute__((aligned(16))) float Bs[2][64];
  typedef typename Vec8<T16>::type frag_t;
  int b, h;
  attn_block_head(H >> 6, true, n_long, b, h);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int q0 = bq0[b], q1 = bq1[b], k0 = bk0[b], k1 = bk1[b];
  int tq[2];
  frag_t qf[2][2];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    tq[qb] = q0 + wave * 32 + qb * 16 + fr;
    const T16* qp = qkv + (size_t)(tq[qb] < q1 ? tq[qb] : q0) * ld + h * 64 + g * 8;
    qf[qb][0] = *reinterpret_cast<const frag_t*>(qp);
    qf[qb][1] = *reinterpret_cast<const frag_t*>(qp + 32);
  }
  float m[2] = {-1e30f, -1e30f}, l[2] = {0.f, 0.f};
  f32x4_t o[2][4];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[qb][dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int srow = tid >> 2, sc0 = (tid & 3) * 2;       // staging: row 0..63, two 16-byte chunks of K and of V
  uint4 kv[2], vv[2];
  float bv = 0.f;
  auto gload = [&](int kt) {
    if (kt + srow < k1) {
      const T16* kp = qkv + (size_t)(kt + srow) * ld + H + h * 64 + sc0 * 8;
      kv[0] = *reinterpret_cast<const uint4*>(kp);
      kv[1] = *reinterpret_cast<const uint4*>(kp + 8);
      vv[0] = *reinterpret_cast<const uint4*>(kp + H);
      vv[1] = *reinterpret_cast<const uint4*>(kp + H + 8);
    } else {
      kv[0] = kv[1] = vv[0] = vv[1] = make_uint4(0, 0, 0, 0);
    }
    if (tid < 64) bv = (kt + tid < k1) ? (key_bias ? key_bias[kt + tid] : 0.f) : -1e30f;
  };
  auto lstore = [&](int d) {
    *reinterpret_cast<uint4*>(Ks[d] + srow * RS + sc0 * 16) = kv[0];
    *reinterpret_cast<uint4*>(Ks[d] + srow * RS + sc0 * 16 + 16) = kv[1];
    *reinterpret_cast<uint4*>(Vs[d] + srow * RS + sc0 * 16) = vv[0];
    *reinterpret_cast<uint4*>(Vs[d] + srow * RS + sc0 * 16 + 16) = vv[1];
    if (tid < 64) Bs[d][tid] = bv;
  };
  gload(k0);
  lstore(0);
  __syncthreads();
  int d = 0;
  for (int kt = k0; kt < k1; kt += 64, d ^= 1) {
    const bool more = kt + 64 < k1;
    if (more) gload(kt + 64);
    const bool biased = key_bias != nullptr || kt + 64 > k1;       // uniform: otherwise the staged bias is all zero
    f32x4_t sacc[2][4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      sacc[0][it] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
      sacc[1][it] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const frag_t kf = *reinterpret_cast<const frag_t*>(Ks[d] + (it * 16 + fr) * RS + (ks * 32 + g * 8) * 2);
        sacc[0][it] = mfma_16x16x32(kf, qf[0][ks], sacc[0][it]);
        sacc[1][it] = mfma_16x16x32(kf, qf[1][ks], sacc[1][it]);
      }
    }
    // sacc[qb][it][r] = score(key kt + it*16 + g*4 + r, query block qb column fr)
    if (biased) {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const f32x4_t bb = *reinterpret_cast<const f32x4_t*>(&Bs[d][it * 16 + g * 4]);
        sacc[0][it] += bb;
        sacc[1][it] += bb;
      }
    }
    frag_t pf[2][2];
    flash_softmax_step<T16>(sacc[0], m[0], l[0], o[0], pf[0]);
    flash_softmax_step<T16>(sacc[1], m[1], l[1], o[1], pf[1]);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const char* base = Vs[d] + (32 * s2 + 4 * g + (fr >> 2)) * RS + (dt * 16 + (fr & 3) * 4) * 2;
        union { struct { tr16x4_t a, b; } s; frag_t f; } u;
        u.s.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)base);
        u.s.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(base + 16 * RS));
        o[0][dt] = mfma_16x16x32(u.f, pf[0][s2], o[0][dt]);
        o[1][dt] = mfma_16x16x32(u.f, pf[1][s2], o[1][dt]);
      }
    if (more) lstore(d ^ 1);     // that buffer's last readers passed the barrier that ended the previous iteration
    __syncthreads();
  }
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
    if (tq[qb] < q1) {
      const float inv = 1.0f / l[qb];
      T16* op = ctx + (size_t)tq[qb] * ldc + h * 64 + g * 4;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) store4(op + dt * 16, o[qb][dt] * inv);
    }
}

// ---------------------------------------------------------------------------------------------
// Sub-word pooling fused with the layer mix.
//   out[dst_row[w]][:] = sum_l wl[l] * mean_{p in [start, start+len)} layer_l[p][:]
// One workgroup per word, its four waves share the layers (wave v takes layers v*ceil(NL/4) ...), every wave issues the
// loads of up to three layers x two pieces x H/256 column groups (18 x 16 B per lane at bert-base) BEFORE it touches any of
// them, and the four partial rows meet in LDS.  A word is 12-24 rows of 1.5-4 KB scattered over as many layer matrices, so
// the kernel lives on bytes in flight: the first version (one wave per word, one layer per loop trip, three 8-byte loads
// outstanding) ran at 1.4-1.6 TB/s.  All loads are unconditional (an out-of-range layer / piece re-reads a valid row with
// weight 0): hipcc turns a per-load runtime condition into a branch plus s_waitcnt vmcnt(0) per load.
// ---------------------------------------------------------------------------------------------
#define POOL_MAX_LAYERS 32
#define POOL_LPB 3
template <typename T, int NG>
__global__ __launch_bounds__(256) void pool_mix_kernel(const T* __restrict__ layers, size_t layer_stride, int ldl, int NL,
                                                       const int* __restrict__ span_start, const int* __restrict__ span_start_last,
                                                       const int* __restrict__ span_len,
                                                       const int* __restrict__ dst_row, const float* __restrict__ wl,
                                                       float* __restrict__ out, int ldo, int W, int H) {
  __shared__ __attribute__((aligned(16))) float red[3][NG * 256];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int w = blockIdx.x;
  const int st = span_start[w], n = span_len[w];
  const int st_last = span_start_last ? span_start_last[w] : st;        // the last layer may be stored compacted (pooled rows only)
  const float inv = 1.0f / (float)n;
  const int per = (NL + 3) >> 2;
  const int l0 = wv * per, l1 = min(NL, l0 + per);
  f32x4_t acc[NG];
  int col[NG];                                          // a lane past the row's end (H not a multiple of 256) re-reads the last group
#pragma unroll
  for (int i = 0; i < NG; ++i) {
    acc[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    col[i] = min((i * 64 + lane) * 4, H - 4);
  }
  // n is the same for the whole workgroup: one-piece words (half of them at ST-VQA item lengths) take the path without the second
  // row's loads (the first version loaded piece 0 twice with weight 0: a quarter of the kernel's L2 traffic for nothing)
  auto body = [&](auto two_tag) {
    constexpr bool TWO = decltype(two_tag)::value;
    for (int lb = l0; lb < l1; lb += POOL_LPB) {
      f32x4_t v[POOL_LPB][TWO ? 2 : 1][NG];
      float wgt[POOL_LPB];
#pragma unroll
      for (int j = 0; j < POOL_LPB; ++j) {
        const int l = min(lb + j, l1 - 1);
        wgt[j] = (lb + j < l1) ? wl[l] * inv : 0.f;
        const T* base = layers + (size_t)l * layer_stride + (size_t)(l == NL - 1 ? st_last : st) * ldl;
#pragma unroll
        for (int i = 0; i < NG; ++i) {
          v[j][0][i] = load4_stream(base + col[i]);
          if (TWO) v[j][TWO ? 1 : 0][i] = load4_stream(base + (size_t)ldl + col[i]);
        }
      }
#pragma unroll
      for (int j = 0; j < POOL_LPB; ++j)
#pragma unroll
        for (int i = 0; i < NG; ++i) acc[i] += (TWO ? v[j][0][i] + v[j][TWO ? 1 : 0][i] : v[j][0][i]) * wgt[j];
      if (TWO && n > 2) {                                 // rare: words of three or more pieces
        for (int j = 0; j < POOL_LPB && lb + j < l1; ++j) {
          const T* base = layers + (size_t)(lb + j) * layer_stride + (size_t)(lb + j == NL - 1 ? st_last : st) * ldl;
          for (int p = 2; p < n; ++p)
#pragma unroll
            for (int i = 0; i < NG; ++i) acc[i] += load4_stream(base + (size_t)p * ldl + col[i]) * wgt[j];
        }
      }
    }
  };
  if (n > 1) body(std::true_type{});
  else body(std::false_type{});
  if (wv > 0) {
#pragma unroll
    for (int i = 0; i < NG; ++i) *reinterpret_cast<f32x4_t*>(&red[wv - 1][(i * 64 + lane) * 4]) = acc[i];
  }
  __syncthreads();
  if (wv == 0) {
    float* o = out + (size_t)dst_row[w] * ldo;
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      const int c = (i * 64 + lane) * 4;
      f32x4_t r = acc[i];
#pragma unroll
      for (int k = 0; k < 3; ++k) r += *reinterpret_cast<const f32x4_t*>(&red[k][c]);
      if (c < H) store4(o + c, r);
    }
  }
}

// The same op with the workgroup cut along the COLUMNS instead of the layers: wave g owns columns 256 g .. 256 g + 255 of the word's row
// for all layers, so nothing is exchanged - no LDS image, no barrier, no wave waiting for the slowest of four (the layer-split form
// above sits at 3.1 TB/s against 4.6 for its own backward, which has the same reads and no cross-wave sum).  Six layers' loads (x one
// or two pieces) are in flight per lane at a time.  Used when H is a multiple of 256 (bert-base / bert-large).
template <typename T>
__global__ __launch_bounds__(256) void pool_mix_cols_kernel(const T* __restrict__ layers, size_t layer_stride, int ldl, int NL,
                                                            const int* __restrict__ span_start, const int* __restrict__ span_start_last,
                                                            const int* __restrict__ span_len, const int* __restrict__ dst_row,
                                                            const float* __restrict__ wl, float* __restrict__ out, int ldo, int W, int H) {
#define RUART_POOL_LB 6
  constexpr int LB = RUART_POOL_LB;
  const int w = blockIdx.x;
  const int st = span_start[w], n = span_len[w];
  const int st_last = span_start_last ? span_start_last[w] : st;
  const float inv = 1.0f / (float)n;
  const int col = threadIdx.x * 4;                       // blockDim.x = H / 4
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  auto body = [&](auto two_tag) {
    constexpr bool TWO = decltype(two_tag)::value;
    for (int lb = 0; lb < NL; lb += LB) {
      f32x4_t v[LB][TWO ? 2 : 1];
      float wgt[LB];
#pragma unroll
      for (int j = 0; j < LB; ++j) {
        const int l = min(lb + j, NL - 1);
        wgt[j] = (lb + j < NL) ? wl[l] * inv : 0.f;
        const T* base = layers + (size_t)l * layer_stride + (size_t)(l == NL - 1 ? st_last : st) * ldl + col;
        v[j][0] = load4_stream(base);
        if (TWO) v[j][TWO ? 1 : 0] = load4_stream(base + (size_t)ldl);
      }
#pragma unroll
      for (int j = 0; j < LB; ++j) acc += (TWO ? v[j][0] + v[j][TWO ? 1 : 0] : v[j][0]) * wgt[j];
      if (TWO && n > 2) {
        for (int j = 0; j < LB && lb + j < NL; ++j) {
          const T* base = layers + (size_t)(lb + j) * layer_stride + (size_t)(lb + j == NL - 1 ? st_last : st) * ldl + col;
          for (int p = 2; p < n; ++p) acc += load4_stream(base + (size_t)p * ldl) * wgt[j];
        }
      }
    }
  };
  if (n > 1) body(std::true_type{});
  else body(std::false_type{});
  store4(out + (size_t)dst_row[w] * ldo + col, acc);
}

// d(loss)/d(wl[l]) partial of one word: <grad_out[dst_row[w]], mean of the word's rows of layer l>; partial[w * NL + l].
template <typename T, int NG>
__global__ __launch_bounds__(256) void pool_mix_bwd_kernel(const T* __restrict__ layers, size_t layer_stride, int ldl, int NL,
                                                           const int* __restrict__ span_start, const int* __restrict__ span_start_last,
                                                           const int* __restrict__ span_len,
                                                           const int* __restrict__ dst_row, const float* __restrict__ gout, int ldg,
                                                           float* __restrict__ partial, int W, int H) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int w = blockIdx.x;
  const int st = span_start[w], n = span_len[w];
  const int st_last = span_start_last ? span_start_last[w] : st;        // the last layer may be stored compacted (pooled rows only)
  const float inv = 1.0f / (float)n;
  const int per = (NL + 3) >> 2;
  const int l0 = wv * per, l1 = min(NL, l0 + per);
  f32x4_t gv[NG];
  int col[NG];
  const float* g = gout + (size_t)dst_row[w] * ldg;
#pragma unroll
  for (int i = 0; i < NG; ++i) {
    const int c = (i * 64 + lane) * 4;
    col[i] = min(c, H - 4);
    gv[i] = load4(g + col[i]);
    if (c >= H) gv[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};   // lanes past the row's end contribute nothing
  }
  auto body = [&](auto two_tag) {                        // see pool_mix_kernel: one-piece words skip the second row's loads
    constexpr bool TWO = decltype(two_tag)::value;
    for (int lb = l0; lb < l1; lb += POOL_LPB) {
      f32x4_t v[POOL_LPB][TWO ? 2 : 1][NG];
#pragma unroll
      for (int j = 0; j < POOL_LPB; ++j) {
        const int l = min(lb + j, l1 - 1);
        const T* base = layers + (size_t)l * layer_stride + (size_t)(l == NL - 1 ? st_last : st) * ldl;
#pragma unroll
        for (int i = 0; i < NG; ++i) {
          v[j][0][i] = load4_stream(base + col[i]);
          if (TWO) v[j][TWO ? 1 : 0][i] = load4_stream(base + (size_t)ldl + col[i]);
        }
      }
#pragma unroll
      for (int j = 0; j < POOL_LPB; ++j) {
        f32x4_t s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NG; ++i) s4 += (TWO ? v[j][0][i] + v[j][TWO ? 1 : 0][i] : v[j][0][i]) * gv[i];
        if (TWO && n > 2 && lb + j < l1) {
          const T* base = layers + (size_t)(lb + j) * layer_stride + (size_t)(lb + j == NL - 1 ? st_last : st) * ldl;
          for (int p = 2; p < n; ++p)
#pragma unroll
            for (int i = 0; i < NG; ++i) s4 += load4_stream(base + (size_t)p * ldl + col[i]) * gv[i];
        }
        const float d = wave_sum(s4[0] + s4[1] + s4[2] + s4[3]) * inv;
        if (lane == 0 && lb + j < l1) partial[(size_t)w * NL + lb + j] = d;
      }
    }
  };
  if (n > 1) body(std::true_type{});
  else body(std::false_type{});
}

__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ partial, int nrows, int NL, float* __restrict__ out) {
  // one workgroup per layer weight; fixed summation order => bitwise reproducible
  __shared__ float red[4];
  const int l = blockIdx.x;
  float s = 0.f;
  for (int b = threadIdx.x; b < nrows; b += 256) s += partial[(size_t)b * NL + l];
  s = block_sum<4>(s, red);
  if (threadIdx.x == 0) out[l] = s;
}

template <typename TIn, typename TOut>
__global__ void cast_kernel(const TIn* __restrict__ in, TOut* __restrict__ out, size_t n4, float scale) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    f32x4_t v = load4(in + i * 4);
    store4(out + i * 4, v * scale);
  }
}

// ---------------------------------------------------------------------------------------------
extern "C" int ruart_rows_layernorm(const float* x, int ldx, const float* gamma, const float* beta, float eps, void* out, int ldo,
                                    int out_dtype, int rows, int H, void* stream) {
  RUART_ENTRY();
  if (H % 4 || H > 256 * MAXG || rows <= 0 || (ldx & 3) || (ldo & 3)) return (int)hipErrorInvalidValue;
  const dim3 grid(ceil_div(rows, 4)), block(256);
  if (out_dtype == RUART_DT_BF16)
    hipLaunchKernelGGL(rows_layernorm_kernel<bf16_t>, grid, block, 0, (hipStream_t)stream, x, ldx, gamma, beta, eps, (bf16_t*)out, ldo, rows, H);
  else if (out_dtype == RUART_DT_F16)
    hipLaunchKernelGGL(rows_layernorm_kernel<f16_t>, grid, block, 0, (hipStream_t)stream, x, ldx, gamma, beta, eps, (f16_t*)out, ldo, rows, H);
  else
    hipLaunchKernelGGL(rows_layernorm_kernel<float>, grid, block, 0, (hipStream_t)stream, x, ldx, gamma, beta, eps, (float*)out, ldo, rows, H);
  RUART_CHECK_LAUNCH();
  return 0;
}

static const bool g_attn_split_valu = getenv("RUART_ATTN_SPLIT_VALU") != nullptr;
// heads per workgroup of the split attention kernel: 2 = the multi-head form with the next head's loads in flight (bit-identical to the
// one-head kernel; on the bench stream 124 against 131 us per call with the non-temporal loads, equal inside a whole pass - DESIGN.md section 5)
static int g_attn_split_hpg = getenv("RUART_ATTN_SPLIT_HEADS") ? atoi(getenv("RUART_ATTN_SPLIT_HEADS")) : 2;

extern "C" int ruart_rows_layernorm_split(const float* x, int ldx, const float* gamma, const float* beta, float eps, float* out32,
                                          void* out16, void* out8, int ldo, int rows, int H, void* stream) {
  RUART_ENTRY();
  if (H % 4 || H > 256 * MAXG || rows <= 0 || (ldx & 3) || (ldo & 3) || !out32 || !out16 || !out8) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(rows_layernorm_split_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, ldx, gamma, beta, eps, out32,
                     (f16_t*)out16, (unsigned char*)out8, ldo, rows, H);
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_bert_embed_ln_split(const int* ids, const int* pos, const float* word_emb, const float* pos_emb, const float* type_emb,
                                         const float* gamma, const float* beta, float eps, float* out32, void* out16, void* out8, int ldo,
                                         int rows, int H, void* stream) {
  RUART_ENTRY();
  if (H % 4 || H > 256 * MAXG || rows <= 0 || (ldo & 3) || !out32 || !out16 || !out8) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(embed_ln_split_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream, ids, pos, word_emb, pos_emb, type_emb,
                     gamma, beta, eps, out32, (f16_t*)out16, (unsigned char*)out8, ldo, rows, H);
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_bert_attention_split(const float* qkv, int ld, void* ctx16, void* ctx8, int ldc, int H, int n_heads, int n_blocks,
                                          const int* blk_q0, const int* blk_q1, const int* blk_k0, const int* blk_k1, const int* tok_lo,
                                          const int* tok_hi, const float* key_bias, void* stream) {
  RUART_ENTRY();
  if (n_heads * 64 != H || n_blocks <= 0 || !ctx16 || !ctx8 || (ldc & 3)) return (int)hipErrorInvalidValue;
  if (g_attn_split_valu)       // diagnostic: the fp32 VALU kernel (lane = query) instead of the split-f16 MFMA kernel
    hipLaunchKernelGGL((attn_varlen_kernel<float, true>), dim3(n_blocks, n_heads), dim3(64), 0, (hipStream_t)stream, qkv, ld, (float*)nullptr,
                       ldc, H, blk_q0, blk_q1, blk_k0, blk_k1, tok_lo, tok_hi, key_bias, (f16_t*)ctx16, (unsigned char*)ctx8);
  else {
    // heads per workgroup: g_attn_split_hpg (ruart_bert_attention_split_set_heads; 0 = the one-head kernel), lowered to a divisor of n_heads
    int hpg = g_attn_split_hpg;
    while (hpg > 1 && n_heads % hpg) --hpg;
#define RUART_MH(N) hipLaunchKernelGGL(attn_flash_split_mh_kernel<N>, dim3((unsigned)n_blocks * (unsigned)(n_heads / N)), dim3(256), 0,  \
                                       (hipStream_t)stream, qkv, ld, (f16_t*)ctx16, (unsigned char*)ctx8, ldc, H, blk_q0, blk_q1, blk_k0, blk_k1, \
                                       tok_lo, key_bias)
    switch (hpg) {
      case 2: RUART_MH(2); break;
      case 3: RUART_MH(3); break;
      case 4: RUART_MH(4); break;
      case 6: RUART_MH(6); break;
      case 8: RUART_MH(8); break;
      case 12: RUART_MH(12); break;
      case 16: RUART_MH(16); break;
      default:
        hipLaunchKernelGGL(attn_flash_split_kernel, attn_grid(n_blocks, n_heads), dim3(256), 0, (hipStream_t)stream, qkv, ld, (f16_t*)ctx16,
                           (unsigned char*)ctx8, ldc, H, blk_q0, blk_q1, blk_k0, blk_k1, tok_lo, key_bias);
    }
#undef RUART_MH
  }
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_bert_attention_split_set_heads(int heads_per_workgroup) {
  RUART_ENTRY();
  if (heads_per_workgroup < 0 || heads_per_workgroup > 16) return (int)hipErrorInvalidValue;
  g_attn_split_hpg = heads_per_workgroup;
  return 0;
}

extern "C" int ruart_bert_embed_ln(const int* ids, const int* pos, const float* word_emb, const float* pos_emb,
                                   const float* type_emb, const float* gamma, const float* beta, float eps, void* out, int ldo,
                                   int out_dtype, int rows, int H, void* stream) {
  RUART_ENTRY();
  if (H % 4 || H > 256 * MAXG || rows <= 0 || (ldo & 3)) return (int)hipErrorInvalidValue;
  const dim3 grid(ceil_div(rows, 4)), block(256);
  if (out_dtype == RUART_DT_BF16)
    hipLaunchKernelGGL(embed_ln_kernel<bf16_t>, grid, block, 0, (hipStream_t)stream, ids, pos, word_emb, pos_emb, type_emb, gamma, beta, eps, (bf16_t*)out, ldo, rows, H);
  else if (out_dtype == RUART_DT_F16)
    hipLaunchKernelGGL(embed_ln_kernel<f16_t>, grid, block, 0, (hipStream_t)stream, ids, pos, word_emb, pos_emb, type_emb, gamma, beta, eps, (f16_t*)out, ldo, rows, H);
  else
    hipLaunchKernelGGL(embed_ln_kernel<float>, grid, block, 0, (hipStream_t)stream, ids, pos, word_emb, pos_emb, type_emb, gamma, beta, eps, (float*)out, ldo, rows, H);
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_bert_attention(const void* qkv, int ld, void* ctx, int ldc, int dtype, int H, int n_heads, int n_blocks,
                                    const int* blk_q0, const int* blk_q1, const int* blk_k0, const int* blk_k1,
                                    const int* tok_lo, const int* tok_hi, const float* key_bias, int n_long_blocks,
                                    const int* lblk_q0, const int* lblk_q1, const int* lblk_k0, const int* lblk_k1, void* stream) {
  RUART_ENTRY();
  if (n_heads * 64 != H || n_blocks < 0 || n_long_blocks < 0 || n_blocks + n_long_blocks <= 0) return (int)hipErrorInvalidValue;
  if (n_long_blocks > 0 && dtype == RUART_DT_F32) return (int)hipErrorInvalidValue;   // the MFMA kernel is 16-bit only
  hipStream_t st = (hipStream_t)stream;
  if (dtype == RUART_DT_F32) {
    if (n_blocks > 0) {
      hipLaunchKernelGGL(attn_varlen_kernel<float>, dim3(n_blocks, n_heads), dim3(64), 0, st, (const float*)qkv, ld, (float*)ctx, ldc, H, blk_q0, blk_q1, blk_k0, blk_k1, tok_lo, tok_hi, key_bias);
      RUART_CHECK_LAUNCH();
    }
    return 0;
  }
  // 16-bit: MFMA kernels.  Short windows are a one-tile call with a block-diagonal mask; long sequences come as blocks of up to
  // 128 queries that see the whole sequence.
  if (n_blocks > 0) {
    const dim3 grid = attn_grid(n_blocks, n_heads), block(256);
    if (dtype == RUART_DT_BF16)
      hipLaunchKernelGGL(attn_flash_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)qkv, ld, (bf16_t*)ctx, ldc, H, blk_q0, blk_q1, blk_k0, blk_k1, tok_lo, key_bias);
    else
      hipLaunchKernelGGL(attn_flash_kernel<f16_t>, grid, block, 0, st, (const f16_t*)qkv, ld, (f16_t*)ctx, ldc, H, blk_q0, blk_q1, blk_k0, blk_k1, tok_lo, key_bias);
    RUART_CHECK_LAUNCH();
  }
  if (n_long_blocks > 0) {
    const dim3 grid = attn_grid(n_long_blocks, n_heads), block(256);
    if (dtype == RUART_DT_BF16)
      hipLaunchKernelGGL(attn_flash_long_kernel<bf16_t>, grid, block, 0, st, (const bf16_t*)qkv, ld, (bf16_t*)ctx, ldc, H, lblk_q0, lblk_q1, lblk_k0, lblk_k1, key_bias, n_long_blocks);
    else
      hipLaunchKernelGGL(attn_flash_long_kernel<f16_t>, grid, block, 0, st, (const f16_t*)qkv, ld, (f16_t*)ctx, ldc, H, lblk_q0, lblk_q1, lblk_k0, lblk_k1, key_bias, n_long_blocks);
    RUART_CHECK_LAUNCH();
  }
  return 0;
}

// ---- pooling over PRE-LayerNorm layer rows (the folded encoder pass, ruart_bert_forward_folded): layer l's output row is
//   (y - mu) rstd gamma_l + beta_l   with (mu, rstd) = stats[l][row], gamma / beta [NL][H]
// and is formed on the fly - per loaded element one fma with the row's (rstd, -mu rstd) and one with the layer's gamma; beta enters once
// per layer (the mean over a word's pieces of a constant).  fp32 rows, H % 256 == 0; otherwise the column-split kernels above.
struct PoolLN {
  const float2* stats;       // [NL][stats_stride] (mu, rstd)
  size_t stats_stride;
  const float* g;            // [NL][H]
  const float* b;
};
__global__ __launch_bounds__(256) void pool_mix_cols_ln_kernel(const float* __restrict__ layers, size_t layer_stride, int ldl, int NL,
                                                               const int* __restrict__ span_start, const int* __restrict__ span_start_last,
                                                               const int* __restrict__ span_len, const int* __restrict__ dst_row,
                                                               const float* __restrict__ wl, float* __restrict__ out, int ldo, int W, int H,
                                                               PoolLN ln) {
  constexpr int LB = 6;
  const int w = blockIdx.x;
  const int st = span_start[w], n = span_len[w];
  const int st_last = span_start_last ? span_start_last[w] : st;
  const float inv = 1.0f / (float)n;
  const int col = threadIdx.x * 4;                       // blockDim.x = H / 4
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  auto body = [&](auto two_tag) {
    constexpr bool TWO = decltype(two_tag)::value;
    for (int lb = 0; lb < NL; lb += LB) {
      f32x4_t v[LB][TWO ? 2 : 1], g[LB], be[LB];
      float2 sa[LB][TWO ? 2 : 1];
      float wgt[LB];
#pragma unroll
      for (int j = 0; j < LB; ++j) {
        const int l = min(lb + j, NL - 1);
        wgt[j] = (lb + j < NL) ? wl[l] : 0.f;
        const int r0 = (l == NL - 1 ? st_last : st);
        const float* base = layers + (size_t)l * layer_stride + (size_t)r0 * ldl + col;
        v[j][0] = load4_stream(base);
        sa[j][0] = ln.stats[(size_t)l * ln.stats_stride + r0];
        if (TWO) {
          v[j][TWO ? 1 : 0] = load4_stream(base + (size_t)ldl);
          sa[j][TWO ? 1 : 0] = ln.stats[(size_t)l * ln.stats_stride + r0 + 1];
        }
        g[j] = load4(ln.g + (size_t)l * H + col);
        be[j] = load4(ln.b + (size_t)l * H + col);
      }
#pragma unroll
      for (int j = 0; j < LB; ++j) {
        f32x4_t x;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          x[r] = (v[j][0][r] - sa[j][0].x) * sa[j][0].y;
          if (TWO) x[r] += (v[j][TWO ? 1 : 0][r] - sa[j][TWO ? 1 : 0].x) * sa[j][TWO ? 1 : 0].y;
        }
        acc += (x * g[j]) * (wgt[j] * inv) + be[j] * wgt[j];
      }
      if (TWO && n > 2) {
        for (int j = 0; j < LB && lb + j < NL; ++j) {
          const int r0 = (lb + j == NL - 1 ? st_last : st);
          const float* base = layers + (size_t)(lb + j) * layer_stride + (size_t)r0 * ldl + col;
          for (int p = 2; p < n; ++p) {
            const float2 s2 = ln.stats[(size_t)(lb + j) * ln.stats_stride + r0 + p];
            const f32x4_t y = load4_stream(base + (size_t)p * ldl);
            f32x4_t x;
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] = (y[r] - s2.x) * s2.y;
            acc += (x * g[j]) * (wgt[j] * inv);
          }
        }
      }
    }
  };
  if (n > 1) body(std::true_type{});
  else body(std::false_type{});
  store4(out + (size_t)dst_row[w] * ldo + col, acc);
}

// The same pooling with the layers' gamma / beta columns held in REGISTERS for WPB words (NLT = the layer count, a compile-time
// constant: bert-base's 12): the two table loads per layer and lane of the kernel above are as many L1 / L2 transactions as the rows
// themselves (236 us over the three groups of the bench batch against 194 for the plain kernel); loaded once per workgroup and reused
// over WPB words they cost a quarter of that.  192 threads (H = 768) x 24 f32x4 = 96 VGPRs of tables.
#define RUART_POOL_LN_WPB 4
template <int NLT>
__global__ __launch_bounds__(256) void pool_mix_cols_ln_reg_kernel(const float* __restrict__ layers, size_t layer_stride, int ldl,
                                                                   const int* __restrict__ span_start, const int* __restrict__ span_start_last,
                                                                   const int* __restrict__ span_len, const int* __restrict__ dst_row,
                                                                   const float* __restrict__ wl, float* __restrict__ out, int ldo, int W, int H,
                                                                   PoolLN ln) {
  constexpr int LB = 6, WPB = RUART_POOL_LN_WPB;
  static_assert(NLT % LB == 0, "layers are loaded six at a time");
  const int col = threadIdx.x * 4;                       // blockDim.x = H / 4
  f32x4_t g[NLT], be[NLT];
  float wgt[NLT];
  f32x4_t bsum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int l = 0; l < NLT; ++l) {
    g[l] = load4(ln.g + (size_t)l * H + col);
    be[l] = load4(ln.b + (size_t)l * H + col);
    wgt[l] = wl[l];
    bsum += be[l] * wgt[l];                              // (the mean over a word's pieces of a constant: once per layer)
  }
  for (int wi = 0; wi < WPB; ++wi) {
    const int w = blockIdx.x * WPB + wi;
    if (w >= W) break;
    const int st = span_start[w], n = span_len[w];
    const int st_last = span_start_last ? span_start_last[w] : st;
    const float inv = 1.0f / (float)n;
    f32x4_t acc = bsum;
    // The (mu, rstd) pairs are wave-uniform (word, layer, piece): the compiler turns these into SCALAR loads (s_load_dwordx2 / x4
    // through the scalar cache) - no vector-memory slot, no broadcast.  (A form that fetched the word's 24 pairs with ONE vector load
    // per lane and read them back with v_readlane was 6 % faster and WRONG under load: the scores of a three-stream forward differed
    // from the one-stream forward's by up to 1e-3 from run to run, tools/r05_race_probe.py.  Round 5 blamed an early read of the load;
    // round 6 refuted that - its counted wait was right, loads of both cache policies return in issue order
    // (tools/r06_load_order_probe.hip), a full vmcnt(0) changes nothing - and found that the fault follows the BUILD of that
    // kernel: clean with the values moved to VGPRs (ds_bpermute, or v_mov behind the v_readlane) and clean when the same source is
    // compiled with -fno-slp-vectorize; DESIGN.md section 5, profiles/r06_readlane_diag.log.  The form stays out.)
    auto stat_of = [&](int l, int p) { return ln.stats[(size_t)l * ln.stats_stride + (l == NLT - 1 ? st_last : st) + min(p, n - 1)]; };
    auto body = [&](auto two_tag) {
      constexpr bool TWO = decltype(two_tag)::value;
#pragma unroll
      for (int lb = 0; lb < NLT; lb += LB) {
        f32x4_t v[LB][TWO ? 2 : 1];
#pragma unroll
        for (int j = 0; j < LB; ++j) {
          const int l = lb + j;
          const int r0 = (l == NLT - 1 ? st_last : st);
          const float* base = layers + (size_t)l * layer_stride + (size_t)r0 * ldl + col;
          v[j][0] = load4_stream(base);
          if (TWO) v[j][TWO ? 1 : 0] = load4_stream(base + (size_t)ldl);
        }
#pragma unroll
        for (int j = 0; j < LB; ++j) {
          const float2 s0 = stat_of(lb + j, 0), s1 = stat_of(lb + j, TWO ? 1 : 0);
          f32x4_t x;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            x[r] = (v[j][0][r] - s0.x) * s0.y;
            if (TWO) x[r] += (v[j][TWO ? 1 : 0][r] - s1.x) * s1.y;
          }
          acc += (x * g[lb + j]) * (wgt[lb + j] * inv);
        }
        if (TWO && n > 2) {
#pragma unroll
          for (int j = 0; j < LB; ++j) {
            const int r0 = (lb + j == NLT - 1 ? st_last : st);
            const float* base = layers + (size_t)(lb + j) * layer_stride + (size_t)r0 * ldl + col;
            for (int p = 2; p < n; ++p) {
              const float2 s2 = ln.stats[(size_t)(lb + j) * ln.stats_stride + r0 + p];
              const f32x4_t y = load4_stream(base + (size_t)p * ldl);
              f32x4_t x;
#pragma unroll
              for (int r = 0; r < 4; ++r) x[r] = (y[r] - s2.x) * s2.y;
              acc += (x * g[lb + j]) * (wgt[lb + j] * inv);
            }
          }
        }
      }
    };
    if (n > 1) body(std::true_type{});
    else body(std::false_type{});
    store4(out + (size_t)dst_row[w] * ldo + col, acc);
  }
}

// d(loss)/d(wl[l]) partial of one word over pre-LayerNorm rows: <grad_out[dst_row[w]], gamma_l (mean of the word's normalised rows) + beta_l>
template <int NG>
__global__ __launch_bounds__(256) void pool_mix_bwd_ln_kernel(const float* __restrict__ layers, size_t layer_stride, int ldl, int NL,
                                                              const int* __restrict__ span_start, const int* __restrict__ span_start_last,
                                                              const int* __restrict__ span_len, const int* __restrict__ dst_row,
                                                              const float* __restrict__ gout, int ldg, float* __restrict__ partial, int W, int H,
                                                              PoolLN ln) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int w = blockIdx.x;
  const int st = span_start[w], n = span_len[w];
  const int st_last = span_start_last ? span_start_last[w] : st;
  const float inv = 1.0f / (float)n;
  const int per = (NL + 3) >> 2;
  const int l0 = wv * per, l1 = min(NL, l0 + per);
  f32x4_t gv[NG];
  int col[NG];
  const float* g = gout + (size_t)dst_row[w] * ldg;
#pragma unroll
  for (int i = 0; i < NG; ++i) {
    col[i] = (i * 64 + lane) * 4;                        // H % 256 == 0: every lane inside the row
    gv[i] = load4(g + col[i]);
  }
  for (int l = l0; l < l1; ++l) {
    const int r0 = (l == NL - 1 ? st_last : st);
    const float* base = layers + (size_t)l * layer_stride + (size_t)r0 * ldl;
    f32x4_t x[NG];
#pragma unroll
    for (int i = 0; i < NG; ++i) x[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < n; ++p) {
      const float2 s2 = ln.stats[(size_t)l * ln.stats_stride + r0 + p];
#pragma unroll
      for (int i = 0; i < NG; ++i) {
        const f32x4_t y = load4_stream(base + (size_t)p * ldl + col[i]);
#pragma unroll
        for (int r = 0; r < 4; ++r) x[i][r] += (y[r] - s2.x) * s2.y;
      }
    }
    f32x4_t s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      const f32x4_t gg = load4(ln.g + (size_t)l * H + col[i]), bb = load4(ln.b + (size_t)l * H + col[i]);
      s4 += ((x[i] * gg) * inv + bb) * gv[i];
    }
    const float d = wave_sum((s4[0] + s4[1]) + (s4[2] + s4[3]));
    if (lane == 0) partial[(size_t)w * NL + l] = d;
  }
}

// The backward with the tables in registers as well: wave v owns layers v * NLT / 4 .. (NLT / 4 layers x NG column groups x gamma / beta
// = 72 VGPRs at bert-base), WPB words per workgroup.
template <int NG, int NLT>
__global__ __launch_bounds__(256) void pool_mix_bwd_ln_reg_kernel(const float* __restrict__ layers, size_t layer_stride, int ldl,
                                                                  const int* __restrict__ span_start, const int* __restrict__ span_start_last,
                                                                  const int* __restrict__ span_len, const int* __restrict__ dst_row,
                                                                  const float* __restrict__ gout, int ldg, float* __restrict__ partial, int W, int H,
                                                                  PoolLN ln) {
  constexpr int PER = NLT / 4, WPB = RUART_POOL_LN_WPB;
  static_assert(NLT % 4 == 0, "the four waves share the layers evenly");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int l0 = wv * PER;
  f32x4_t gg[PER][NG], bb[PER][NG];
  int col[NG];
#pragma unroll
  for (int i = 0; i < NG; ++i) col[i] = (i * 64 + lane) * 4;
#pragma unroll
  for (int k = 0; k < PER; ++k)
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      gg[k][i] = load4(ln.g + (size_t)(l0 + k) * H + col[i]);
      bb[k][i] = load4(ln.b + (size_t)(l0 + k) * H + col[i]);
    }
  for (int wi = 0; wi < WPB; ++wi) {
    const int w = blockIdx.x * WPB + wi;
    if (w >= W) break;
    const int st = span_start[w], n = span_len[w];
    const int st_last = span_start_last ? span_start_last[w] : st;
    const float inv = 1.0f / (float)n;
    f32x4_t gv[NG];
    const float* g = gout + (size_t)dst_row[w] * ldg;
#pragma unroll
    for (int i = 0; i < NG; ++i) gv[i] = load4(g + col[i]);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int l = l0 + k;
      const int r0 = (l == NLT - 1 ? st_last : st);
      const float* base = layers + (size_t)l * layer_stride + (size_t)r0 * ldl;
      f32x4_t x[NG];
#pragma unroll
      for (int i = 0; i < NG; ++i) x[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
      for (int p = 0; p < n; ++p) {
        const float2 s2 = ln.stats[(size_t)l * ln.stats_stride + r0 + p];
#pragma unroll
        for (int i = 0; i < NG; ++i) {
          const f32x4_t y = load4_stream(base + (size_t)p * ldl + col[i]);
#pragma unroll
          for (int r = 0; r < 4; ++r) x[i][r] += (y[r] - s2.x) * s2.y;
        }
      }
      f32x4_t s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < NG; ++i) s4 += ((x[i] * gg[k][i]) * inv + bb[k][i]) * gv[i];
      const float d = wave_sum((s4[0] + s4[1]) + (s4[2] + s4[3]));
      if (lane == 0) partial[(size_t)w * NLT + l] = d;
    }
  }
}

// (mu, rstd) of `rows` rows from their partial (sum, sumsq) slots (gemm_corr.hip: four slots of 8 bytes per row, the first np used)
__global__ __launch_bounds__(256) void rows_stats_finish_kernel(const float* __restrict__ part, int np, int rows, float inv_h, float eps,
                                                                float2* __restrict__ stats) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const f32x4_t a = load4(part + (size_t)r * 8), b = load4(part + (size_t)r * 8 + 4);
  const float ps[4] = {a[0], a[2], b[0], b[2]}, pq[4] = {a[1], a[3], b[1], b[3]};
  float s = 0.f, q = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < np) {
      s += ps[k];
      q += pq[k];
    }
  const float mu = s * inv_h;
  const float var = fmaxf(q * inv_h - mu * mu, 0.f);
  stats[r] = make_float2(mu, 1.0f / sqrtf(var + eps));
}
extern "C" int ruart_rows_stats_finish(const float* part, int np, int rows, float inv_h, float eps, float* stats, void* stream) {
  RUART_ENTRY();
  if (!part || !stats || np <= 0 || np > 4 || rows <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(rows_stats_finish_kernel, dim3(ceil_div(rows, 256)), dim3(256), 0, (hipStream_t)stream, part, np, rows, inv_h, eps,
                     (float2*)stats);
  RUART_CHECK_LAUNCH();
  return 0;
}

// row pitches of the pooling entry points: every row is read / written in 8- and 16-byte vectors from column 0
static inline bool pool_pitch_ok(int ld, int H) { return ld >= H && ld % 4 == 0; }

static int g_pool_ln_reg = 1;      // 1: twelve-layer encoders take the register-table form of the pooling kernel (0: A/B runs)
extern "C" int ruart_bert_pool_ln_set_variant(int reg_tables) {
  g_pool_ln_reg = reg_tables < 0 ? 0 : (reg_tables > 2 ? 2 : reg_tables);      // 2: the backward's register-table form too (slower, A/B runs)
  return 0;
}
extern "C" int ruart_bert_pool_mix_ln(const float* layers_pre, long long layer_stride, int ldl, int n_layers, const float* ln_stats,
                                      long long stats_stride, const float* ln_gamma, const float* ln_beta, const int* span_start,
                                      const int* span_start_last, const int* span_len, const int* dst_row, const float* layer_w, float* out,
                                      int ldo, int n_words, int H, void* stream) {
  RUART_ENTRY();
  if (H % 256 || H <= 0 || H > 1024 || n_words <= 0 || n_layers > POOL_MAX_LAYERS || n_layers <= 0 || !ln_stats || !ln_gamma || !ln_beta)
    return (int)hipErrorInvalidValue;
  if (!pool_pitch_ok(ldl, H) || !pool_pitch_ok(ldo, H)) return (int)hipErrorInvalidValue;
  const PoolLN ln{(const float2*)ln_stats, (size_t)stats_stride, ln_gamma, ln_beta};
  if (n_layers == 12 && g_pool_ln_reg)
    hipLaunchKernelGGL(pool_mix_cols_ln_reg_kernel<12>, dim3(ceil_div(n_words, RUART_POOL_LN_WPB)), dim3(H / 4), 0, (hipStream_t)stream, layers_pre,
                       (size_t)layer_stride, ldl, span_start, span_start_last, span_len, dst_row, layer_w, out, ldo, n_words, H, ln);
  else
    hipLaunchKernelGGL(pool_mix_cols_ln_kernel, dim3(n_words), dim3(H / 4), 0, (hipStream_t)stream, layers_pre, (size_t)layer_stride, ldl, n_layers,
                       span_start, span_start_last, span_len, dst_row, layer_w, out, ldo, n_words, H, ln);
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_bert_pool_mix_ln_bwd(const float* layers_pre, long long layer_stride, int ldl, int n_layers, const float* ln_stats,
                                          long long stats_stride, const float* ln_gamma, const float* ln_beta, const int* span_start,
                                          const int* span_start_last, const int* span_len, const int* dst_row, const float* grad_out, int ldg,
                                          float* partial_ws, float* grad_layer_w, int n_words, int H, void* stream) {
  RUART_ENTRY();
  if (H % 256 || H <= 0 || H > 1024 || n_words <= 0 || n_layers > POOL_MAX_LAYERS || n_layers <= 0 || !ln_stats || !ln_gamma || !ln_beta)
    return (int)hipErrorInvalidValue;
  if (!pool_pitch_ok(ldl, H) || !pool_pitch_ok(ldg, H)) return (int)hipErrorInvalidValue;
  const PoolLN ln{(const float2*)ln_stats, (size_t)stats_stride, ln_gamma, ln_beta};
  if (n_layers == 12 && H == 768 && g_pool_ln_reg == 2) {        // (measured slower than the one-word form: 288 against 279 us; kept for A/B runs, variant 2)
    hipLaunchKernelGGL((pool_mix_bwd_ln_reg_kernel<3, 12>), dim3(ceil_div(n_words, RUART_POOL_LN_WPB)), dim3(256), 0, (hipStream_t)stream, layers_pre,
                       (size_t)layer_stride, ldl, span_start, span_start_last, span_len, dst_row, grad_out, ldg, partial_ws, n_words, H, ln);
  } else {
#define POOL(NG) hipLaunchKernelGGL((pool_mix_bwd_ln_kernel<NG>), dim3(n_words), dim3(256), 0, (hipStream_t)stream, layers_pre, (size_t)layer_stride, ldl, n_layers, span_start, span_start_last, span_len, dst_row, grad_out, ldg, partial_ws, n_words, H, ln)
    switch (H / 256) { case 1: POOL(1); break; case 2: POOL(2); break; case 3: POOL(3); break; default: POOL(4); }
#undef POOL
  }
  RUART_CHECK_LAUNCH();
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(n_layers), dim3(256), 0, (hipStream_t)stream, partial_ws, n_words, n_layers, grad_layer_w);
  RUART_CHECK_LAUNCH();
  return 0;
}

static int g_pool_cols = 1;        // 1: column-split pooling kernel where H % 256 == 0 (default); 0: the layer-split form (A/B runs)
extern "C" int ruart_bert_pool_set_variant(int cols) {
  g_pool_cols = cols ? 1 : 0;
  return 0;
}

template <typename T>
static void launch_pool(const void* layers, long long layer_stride, int ldl, int n_layers, const int* span_start, const int* span_start_last,
                        const int* span_len, const int* dst_row, const float* layer_w, float* out, int ldo, int n_words, int H, hipStream_t st) {
  const dim3 grid(n_words), block(256);
  if (H % 256 == 0 && g_pool_cols) {
    hipLaunchKernelGGL((pool_mix_cols_kernel<T>), grid, dim3(H / 4), 0, st, (const T*)layers, (size_t)layer_stride, ldl, n_layers, span_start,
                       span_start_last, span_len, dst_row, layer_w, out, ldo, n_words, H);
    return;
  }
#define POOL(NG) hipLaunchKernelGGL((pool_mix_kernel<T, NG>), grid, block, 0, st, (const T*)layers, (size_t)layer_stride, ldl, n_layers, span_start, span_start_last, span_len, dst_row, layer_w, out, ldo, n_words, H)
  switch ((H + 255) / 256) { case 1: POOL(1); break; case 2: POOL(2); break; case 3: POOL(3); break; default: POOL(4); }
#undef POOL
}
template <typename T>
static void launch_pool_bwd(const void* layers, long long layer_stride, int ldl, int n_layers, const int* span_start,
                            const int* span_start_last, const int* span_len, const int* dst_row, const float* grad_out, int ldg, float* partial, int n_words, int H, hipStream_t st) {
  const dim3 grid(n_words), block(256);
#define POOL(NG) hipLaunchKernelGGL((pool_mix_bwd_kernel<T, NG>), grid, block, 0, st, (const T*)layers, (size_t)layer_stride, ldl, n_layers, span_start, span_start_last, span_len, dst_row, grad_out, ldg, partial, n_words, H)
  switch ((H + 255) / 256) { case 1: POOL(1); break; case 2: POOL(2); break; case 3: POOL(3); break; default: POOL(4); }
#undef POOL
}

extern "C" int ruart_bert_pool_mix(const void* layers, long long layer_stride, int ldl, int dtype, int n_layers,
                                   const int* span_start, const int* span_start_last, const int* span_len, const int* dst_row,
                                   const float* layer_w, float* out, int ldo, int n_words, int H, void* stream) {
  RUART_ENTRY();
  if (H % 4 || H < 4 || H > 1024 || n_words <= 0 || n_layers > POOL_MAX_LAYERS || n_layers <= 0) return (int)hipErrorInvalidValue;
  if (!pool_pitch_ok(ldl, H) || !pool_pitch_ok(ldo, H)) return (int)hipErrorInvalidValue;
  if (dtype == RUART_DT_BF16)
    launch_pool<bf16_t>(layers, layer_stride, ldl, n_layers, span_start, span_start_last, span_len, dst_row, layer_w, out, ldo, n_words, H, (hipStream_t)stream);
  else if (dtype == RUART_DT_F16)
    launch_pool<f16_t>(layers, layer_stride, ldl, n_layers, span_start, span_start_last, span_len, dst_row, layer_w, out, ldo, n_words, H, (hipStream_t)stream);
  else
    launch_pool<float>(layers, layer_stride, ldl, n_layers, span_start, span_start_last, span_len, dst_row, layer_w, out, ldo, n_words, H, (hipStream_t)stream);
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_bert_pool_mix_bwd(const void* layers, long long layer_stride, int ldl, int dtype, int n_layers,
                                       const int* span_start, const int* span_start_last, const int* span_len, const int* dst_row,
                                       const float* grad_out, int ldg, float* partial_ws, float* grad_layer_w, int n_words, int H,
                                       void* stream) {
  RUART_ENTRY();
  if (H % 4 || H < 4 || H > 1024 || n_words <= 0 || n_layers > POOL_MAX_LAYERS || n_layers <= 0) return (int)hipErrorInvalidValue;
  if (!pool_pitch_ok(ldl, H) || !pool_pitch_ok(ldg, H)) return (int)hipErrorInvalidValue;
  if (dtype == RUART_DT_BF16)
    launch_pool_bwd<bf16_t>(layers, layer_stride, ldl, n_layers, span_start, span_start_last, span_len, dst_row, grad_out, ldg, partial_ws, n_words, H, (hipStream_t)stream);
  else if (dtype == RUART_DT_F16)
    launch_pool_bwd<f16_t>(layers, layer_stride, ldl, n_layers, span_start, span_start_last, span_len, dst_row, grad_out, ldg, partial_ws, n_words, H, (hipStream_t)stream);
  else
    launch_pool_bwd<float>(layers, layer_stride, ldl, n_layers, span_start, span_start_last, span_len, dst_row, grad_out, ldg, partial_ws, n_words, H, (hipStream_t)stream);
  RUART_CHECK_LAUNCH();
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(n_layers), dim3(256), 0, (hipStream_t)stream, partial_ws, n_words, n_layers, grad_layer_w);
  RUART_CHECK_LAUNCH();
  return 0;
}

// dst_k[i] = src_k[rows[i]] for up to three byte matrices: one workgroup (256 lanes x 16 B) per output row and matrix slot
struct GatherArgs {
  const char* src[3];
  char* dst[3];
  long long sp[3], dp[3];
  int bytes[3];
};
__global__ __launch_bounds__(256) void rows_gather_kernel(const int* __restrict__ rows, GatherArgs a) {
  const int i = blockIdx.x, r = rows[i];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (!a.src[k]) break;
    const char* s = a.src[k] + (size_t)r * a.sp[k];
    char* d = a.dst[k] + (size_t)i * a.dp[k];
    for (int o = threadIdx.x * 16; o < a.bytes[k]; o += 256 * 16) *reinterpret_cast<f32x4_t*>(d + o) = *reinterpret_cast<const f32x4_t*>(s + o);
  }
}

extern "C" int ruart_rows_gather(const int* rows, int n, const void* src0, long long sp0, void* dst0, long long dp0, int bytes0, const void* src1,
                                 long long sp1, void* dst1, long long dp1, int bytes1, const void* src2, long long sp2, void* dst2, long long dp2,
                                 int bytes2, void* stream) {
  RUART_ENTRY();
  if (!rows || n <= 0 || !src0 || !dst0) return (int)hipErrorInvalidValue;
  GatherArgs a;
  const void* src[3] = {src0, src1, src2};
  void* dst[3] = {dst0, dst1, dst2};
  const long long sp[3] = {sp0, sp1, sp2}, dp[3] = {dp0, dp1, dp2};
  const int by[3] = {bytes0, bytes1, bytes2};
  for (int k = 0; k < 3; ++k) {
    a.src[k] = (const char*)src[k];
    a.dst[k] = (char*)dst[k];
    a.sp[k] = sp[k];
    a.dp[k] = dp[k];
    a.bytes[k] = by[k];
    if (src[k] && (!dst[k] || by[k] <= 0 || (by[k] & 15) || (sp[k] & 15) || (dp[k] & 15) || ((uintptr_t)src[k] & 15) || ((uintptr_t)dst[k] & 15)))
      return (int)hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(rows_gather_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, rows, a);
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_cast_f32_to_16(const float* in, void* out, int out_dtype, long long n, float scale, void* stream) {
  RUART_ENTRY();
  if (n % 4 || (out_dtype != RUART_DT_BF16 && out_dtype != RUART_DT_F16)) return (int)hipErrorInvalidValue;
  const size_t n4 = (size_t)n / 4;
  const int blocks = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
  if (out_dtype == RUART_DT_BF16)
    hipLaunchKernelGGL((cast_kernel<float, bf16_t>), dim3(blocks > 0 ? blocks : 1), dim3(256), 0, (hipStream_t)stream, in, (bf16_t*)out, n4, scale);
  else
    hipLaunchKernelGGL((cast_kernel<float, f16_t>), dim3(blocks > 0 ? blocks : 1), dim3(256), 0, (hipStream_t)stream, in, (f16_t*)out, n4, scale);
  RUART_CHECK_LAUNCH();
  return 0;
}
