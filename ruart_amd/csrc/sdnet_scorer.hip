// Fused answer scorer of the SDNet trunk: Models/Layers.py:352-432 (GetFinalScores, useES + no_answer branches of the shipped conf)
// with its two BilinearSeqAttn (:435-468) and get_single_score (:421-432) - SURVEY's K14.
//
//   score_i  = x_i . u(i),  u(i) = u2 for the first ES slots (attn2, the ES candidates) and u1 for the OCR slots (attn); -inf where the
//              slot is masked (mask_flag)
//   a        = softmax_i(mask(x_i . uh)),  pooled = sum_i a_i x_i,  s_na = w . pooled + b          (the no-answer score)
//   probs    = softmax([score_0 .. score_{L-1}, s_na])
// u1 = W_attn h0 + b, u2 = W_attn2 h0 + b, uh = W_na h0 + b are three small products the caller takes on ruart_gemm_x3 (with the
// variational-dropout masks of x folded into u1 / u2: (x o m) . u = x . (m o u)).  Unfused this was ~12 launches forward and ~25
// backward around a (B, L, D) broadcast product; here one workgroup per sample does each direction in one launch, x (200 KB per
// sample, L2-resident) read three times, every sum in a fixed order.
#include "common.h"
#include "ruart_hip.h"

#define SC_LMAX 1024
extern int* ruart_nan_flag_ptr;

namespace {

// wave-level dot products of row x_i (D floats, D % 4 == 0) with up to two vectors; lanes stride float4
__device__ __forceinline__ void row_dots(const float* __restrict__ xr, const float* __restrict__ ua, const float* __restrict__ ub, int D,
                                         float& da, float& db) {
  const int lane = threadIdx.x & 63;
  float sa = 0.f, sb = 0.f;
  for (int c = lane * 4; c < D; c += 256) {
    const f32x4_t v = load4(xr + c), a = load4(ua + c), b = load4(ub + c);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sa = fmaf(v[r], a[r], sa);
      sb = fmaf(v[r], b[r], sb);
    }
  }
  da = wave_sum(sa);
  db = wave_sum(sb);
}

__global__ __launch_bounds__(256) void scorer_fwd_kernel(const float* __restrict__ x, const float* __restrict__ u1, const float* __restrict__ u2,
                                                         const float* __restrict__ uh, const float* __restrict__ w, const float* __restrict__ bna,
                                                         const unsigned char* __restrict__ mask, float* __restrict__ probs,
                                                         float* __restrict__ a_out, int L, int D, int ES, int mask_flag,
                                                         int* __restrict__ nan_flag) {
  __shared__ float sc[SC_LMAX + 1], z[SC_LMAX];
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* xb = x + (size_t)b * L * D;
  const float *p1 = u1 + (size_t)b * D, *p2 = u2 + (size_t)b * D, *ph = uh + (size_t)b * D;
  const unsigned char* mb = mask + (size_t)b * L;
  for (int i = wave; i < L; i += 4) {
    float s, zz;
    row_dots(xb + (size_t)i * D, i < ES ? p2 : p1, ph, D, s, zz);
    if (lane == 0) {
      const bool on = mb[i] != 0;
      sc[i] = (mask_flag && !on) ? -INFINITY : s;
      z[i] = on ? zz : -INFINITY;
    }
  }
  __syncthreads();
  // a = softmax(z)
  float mx = -INFINITY;
  for (int i = tid; i < L; i += 256) mx = fmaxf(mx, z[i]);
  mx = block_max<4>(mx, red);
  float sum = 0.f;
  for (int i = tid; i < L; i += 256) sum += __expf(z[i] - mx);
  sum = block_sum<4>(sum, red);
  const float inv = 1.0f / sum;
  __syncthreads();
  for (int i = tid; i < L; i += 256) {
    const float a = __expf(z[i] - mx) * inv;
    z[i] = a;
    a_out[(size_t)b * L + i] = a;
  }
  __syncthreads();
  // pooled[d] = sum_i a_i x_i[d] (rows in order), s_na = w . pooled + b
  float part = 0.f;
  for (int d = tid; d < D; d += 256) {
    float p = 0.f;
    for (int i = 0; i < L; ++i) p = fmaf(z[i], xb[(size_t)i * D + d], p);
    part = fmaf(w[d], p, part);
  }
  part = block_sum<4>(part, red);
  if (tid == 0) sc[L] = part + bna[0];
  __syncthreads();
  // probs = softmax(sc[0..L])
  float m2 = -INFINITY;
  for (int i = tid; i <= L; i += 256) m2 = fmaxf(m2, sc[i]);
  m2 = block_max<4>(m2, red);
  float s2 = 0.f;
  for (int i = tid; i <= L; i += 256) s2 += __expf(sc[i] - m2);
  s2 = block_sum<4>(s2, red);
  const float inv2 = 1.0f / s2;
  bool bad = false;
  for (int i = tid; i <= L; i += 256) {
    const float p = __expf(sc[i] - m2) * inv2;
    probs[(size_t)b * (L + 1) + i] = p;
    bad |= !(p == p);
  }
  if (bad && nan_flag) atomicOr(nan_flag, 1);
}

__global__ __launch_bounds__(256) void scorer_bwd_kernel(const float* __restrict__ x, const float* __restrict__ u1, const float* __restrict__ u2,
                                                         const float* __restrict__ uh, const float* __restrict__ w,
                                                         const float* __restrict__ probs, const float* __restrict__ a_in,
                                                         const float* __restrict__ gprobs, float* __restrict__ gx, float* __restrict__ gu1,
                                                         float* __restrict__ gu2, float* __restrict__ guh, float* __restrict__ gw_part,
                                                         float* __restrict__ gb_part, int L, int D, int ES) {
  __shared__ float ds[SC_LMAX + 1], av[SC_LMAX], dz[SC_LMAX];
  __shared__ float red[4];
  extern __shared__ float dpool[];                       // D floats: d(loss)/d(pooled)
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* xb = x + (size_t)b * L * D;
  const float *p1 = u1 + (size_t)b * D, *p2 = u2 + (size_t)b * D, *ph = uh + (size_t)b * D;
  const float* pb = probs + (size_t)b * (L + 1);
  const float* gb = gprobs + (size_t)b * (L + 1);
  // softmax backward: ds_j = p_j (g_j - sum_k g_k p_k)   (masked slots have p = 0)
  float dot = 0.f;
  for (int i = tid; i <= L; i += 256) dot = fmaf(gb[i], pb[i], dot);
  dot = block_sum<4>(dot, red);
  __syncthreads();
  for (int i = tid; i <= L; i += 256) ds[i] = pb[i] * (gb[i] - dot);
  for (int i = tid; i < L; i += 256) av[i] = a_in[(size_t)b * L + i];
  __syncthreads();
  const float ds_na = ds[L];
  // the no-answer branch: pooled again (rows in order), its gradients to w / b, d(pooled) = ds_na * w
  for (int d = tid; d < D; d += 256) {
    float p = 0.f;
    for (int i = 0; i < L; ++i) p = fmaf(av[i], xb[(size_t)i * D + d], p);
    gw_part[(size_t)b * D + d] = ds_na * p;
    dpool[d] = ds_na * w[d];
  }
  if (tid == 0) gb_part[b] = ds_na;
  __syncthreads();
  // da_i = dpool . x_i ;  dz = a o (da - sum_j a_j da_j)
  for (int i = wave; i < L; i += 4) {
    float da, unused;
    row_dots(xb + (size_t)i * D, dpool, dpool, D, da, unused);
    if (lane == 0) dz[i] = da;
  }
  __syncthreads();
  float adot = 0.f;
  for (int i = tid; i < L; i += 256) adot = fmaf(av[i], dz[i], adot);
  adot = block_sum<4>(adot, red);
  __syncthreads();
  for (int i = tid; i < L; i += 256) dz[i] = av[i] * (dz[i] - adot);
  __syncthreads();
  // gx_i = ds_i u(i) + a_i dpool + dz_i uh
  for (int i = wave; i < L; i += 4) {
    const float* ui = i < ES ? p2 : p1;
    const float s = ds[i], a = av[i], zz = dz[i];
    float* g = gx + ((size_t)b * L + i) * D;
    for (int c = lane * 4; c < D; c += 256) {
      const f32x4_t uv = load4(ui + c), hv = load4(ph + c), dv = *reinterpret_cast<const f32x4_t*>(dpool + c);
      store4(g + c, uv * s + dv * a + hv * zz);
    }
  }
  // gu1 = sum_{i >= ES} ds_i x_i, gu2 = sum_{i < ES} ds_i x_i, guh = sum_i dz_i x_i    (rows in order)
  for (int d = tid; d < D; d += 256) {
    float a1 = 0.f, a2 = 0.f, ah = 0.f;
    for (int i = 0; i < L; ++i) {
      const float v = xb[(size_t)i * D + d];
      if (i < ES) a2 = fmaf(ds[i], v, a2);
      else a1 = fmaf(ds[i], v, a1);
      ah = fmaf(dz[i], v, ah);
    }
    gu1[(size_t)b * D + d] = a1;
    gu2[(size_t)b * D + d] = a2;
    guh[(size_t)b * D + d] = ah;
  }
}


// ---- H pooled heads beside the slot scores (label_yesno: Layers.py:405-416) -------------------------------------------------------
//   a_h     = softmax_i(mask(x_i . uh_h)),  s_h = w_h . sum_i a_hi x_i + bh_h                       h = 0 .. H-1
//   probs   = softmax([s_0 .. s_{nf-1}, score_0 .. score_{L-1}, s_nf .. s_{H-1}])                    (H + L columns)
// The kernels above stay as they are for the shipped conf; these read x as often as they do (forward twice, backward three times),
// whatever H: a row pass takes its 1 + H dot products from one read of the row, a column pass the sums of all heads from one walk
// down the rows.  All LDS is dynamic (16-byte aligned carves): red[4], the H + L scores / their gradients, and per head L floats
// (twice in the backward) plus - backward only - the D floats of d(loss)/d(pooled_h).
__host__ __device__ constexpr int sh_up4(int n) { return (n + 3) & ~3; }
// the backward's layout, which contains the forward's: one rule for both directions (include/ruart_hip.h)
inline size_t scorer_heads_lds_bytes(int L, int D, int H) {
  return sizeof(float) * ((size_t)4 + sh_up4(H + L) + (size_t)2 * H * sh_up4(L) + (size_t)H * D);
}
#define SH_LDS_MAX 65536
// column of head h in probs
__device__ __forceinline__ int head_col(int h, int n_front, int L) { return h < n_front ? h : L + h; }

template <int H>
__global__ __launch_bounds__(256) void scorer_heads_fwd_kernel(const float* __restrict__ x, const float* __restrict__ u1,
                                                               const float* __restrict__ u2, const float* __restrict__ uh,
                                                               const float* __restrict__ w, const float* __restrict__ bh,
                                                               const unsigned char* __restrict__ mask, float* __restrict__ probs,
                                                               float* __restrict__ a_out, int L, int D, int ES, int n_front, int mask_flag,
                                                               int* __restrict__ nan_flag) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Lp = sh_up4(L), W = H + L;
  float* red = smem;
  float* sc = red + 4;                  // W scores in output column order
  float* z = sc + sh_up4(W);            // z[h * Lp + i]: head h's attention logits, then weights
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* xb = x + (size_t)b * L * D;
  const float *p1 = u1 + (size_t)b * D, *p2 = u2 + (size_t)b * D, *ph = uh + (size_t)b * H * D;
  const unsigned char* mb = mask + (size_t)b * L;
  // row pass: the slot score and the H attention logits of row i from one read of x_i
  for (int i = wave; i < L; i += 4) {
    const float* xr = xb + (size_t)i * D;
    const float* ui = i < ES ? p2 : p1;
    float s = 0.f, zz[H];
#pragma unroll
    for (int h = 0; h < H; ++h) zz[h] = 0.f;
    for (int c = lane * 4; c < D; c += 256) {
      const f32x4_t v = load4(xr + c), a = load4(ui + c);
#pragma unroll
      for (int r = 0; r < 4; ++r) s = fmaf(v[r], a[r], s);
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const f32x4_t hv = load4(ph + (size_t)h * D + c);
#pragma unroll
        for (int r = 0; r < 4; ++r) zz[h] = fmaf(v[r], hv[r], zz[h]);
      }
    }
    s = wave_sum(s);
#pragma unroll
    for (int h = 0; h < H; ++h) zz[h] = wave_sum(zz[h]);
    if (lane == 0) {
      const bool on = mb[i] != 0;
      sc[n_front + i] = (mask_flag && !on) ? -INFINITY : s;
#pragma unroll
      for (int h = 0; h < H; ++h) z[h * Lp + i] = on ? zz[h] : -INFINITY;
    }
  }
  __syncthreads();
  // a_h = softmax(z_h): wave h takes head h (H <= 4 waves)
  if (wave < H) {
    float* zh = z + wave * Lp;
    float mx = -INFINITY;
    for (int i = lane; i < L; i += 64) mx = fmaxf(mx, zh[i]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int i = lane; i < L; i += 64) sum += __expf(zh[i] - mx);
    const float inv = 1.0f / wave_sum(sum);
    for (int i = lane; i < L; i += 64) {
      const float a = __expf(zh[i] - mx) * inv;
      zh[i] = a;
      a_out[((size_t)b * H + wave) * L + i] = a;
    }
  }
  __syncthreads();
  // column pass: pooled_h[d] = sum_i a_hi x_i[d] (rows in order) for all heads from one walk, s_h = w_h . pooled_h + bh_h
  float part[H];
#pragma unroll
  for (int h = 0; h < H; ++h) part[h] = 0.f;
  for (int d = tid; d < D; d += 256) {
    float p[H];
#pragma unroll
    for (int h = 0; h < H; ++h) p[h] = 0.f;
    for (int i = 0; i < L; ++i) {
      const float v = xb[(size_t)i * D + d];
#pragma unroll
      for (int h = 0; h < H; ++h) p[h] = fmaf(z[h * Lp + i], v, p[h]);
    }
#pragma unroll
    for (int h = 0; h < H; ++h) part[h] = fmaf(w[(size_t)h * D + d], p[h], part[h]);
  }
#pragma unroll
  for (int h = 0; h < H; ++h) {
    const float t = block_sum<4>(part[h], red);
    if (tid == 0) sc[head_col(h, n_front, L)] = t + bh[h];
  }
  __syncthreads();
  // probs = softmax(sc[0..W))
  float m2 = -INFINITY;
  for (int i = tid; i < W; i += 256) m2 = fmaxf(m2, sc[i]);
  m2 = block_max<4>(m2, red);
  float s2 = 0.f;
  for (int i = tid; i < W; i += 256) s2 += __expf(sc[i] - m2);
  s2 = block_sum<4>(s2, red);
  const float inv2 = 1.0f / s2;
  bool bad = false;
  for (int i = tid; i < W; i += 256) {
    const float p = __expf(sc[i] - m2) * inv2;
    probs[(size_t)b * W + i] = p;
    bad |= !(p == p);
  }
  if (bad && nan_flag) atomicOr(nan_flag, 1);
}

template <int H>
__global__ __launch_bounds__(256) void scorer_heads_bwd_kernel(const float* __restrict__ x, const float* __restrict__ u1,
                                                               const float* __restrict__ u2, const float* __restrict__ uh,
                                                               const float* __restrict__ w, const float* __restrict__ probs,
                                                               const float* __restrict__ a_in, const float* __restrict__ gprobs,
                                                               float* __restrict__ gx, float* __restrict__ gu1, float* __restrict__ gu2,
                                                               float* __restrict__ guh, float* __restrict__ gw_part,
                                                               float* __restrict__ gb_part, int L, int D, int ES, int n_front) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Lp = sh_up4(L), W = H + L;
  float* red = smem;
  float* ds = red + 4;                  // W: d(loss)/d(score), output column order
  float* av = ds + sh_up4(W);           // av[h * Lp + i] = a_hi
  float* dz = av + H * Lp;              // dz[h * Lp + i]: d a_hi, then d(logit)_hi
  float* dpool = dz + H * Lp;           // dpool[h * D + d] = d(loss)/d(pooled_h)[d]   (16-byte aligned: every carve is a multiple of 4 floats)
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* xb = x + (size_t)b * L * D;
  const float *p1 = u1 + (size_t)b * D, *p2 = u2 + (size_t)b * D, *ph = uh + (size_t)b * H * D;
  const float* pb = probs + (size_t)b * W;
  const float* gb = gprobs + (size_t)b * W;
  // softmax backward: ds_j = p_j (g_j - sum_k g_k p_k)   (masked slots have p = 0)
  float dot = 0.f;
  for (int i = tid; i < W; i += 256) dot = fmaf(gb[i], pb[i], dot);
  dot = block_sum<4>(dot, red);
  __syncthreads();
  for (int i = tid; i < W; i += 256) ds[i] = pb[i] * (gb[i] - dot);
  for (int j = tid; j < H * L; j += 256) av[(j / L) * Lp + j % L] = a_in[(size_t)b * H * L + j];
  __syncthreads();
  float dsh[H];
#pragma unroll
  for (int h = 0; h < H; ++h) dsh[h] = ds[head_col(h, n_front, L)];
  // column pass 1: pooled_h again (rows in order), its gradients to w_h / bh_h, d(pooled_h) = ds_h * w_h
  for (int d = tid; d < D; d += 256) {
    float p[H];
#pragma unroll
    for (int h = 0; h < H; ++h) p[h] = 0.f;
    for (int i = 0; i < L; ++i) {
      const float v = xb[(size_t)i * D + d];
#pragma unroll
      for (int h = 0; h < H; ++h) p[h] = fmaf(av[h * Lp + i], v, p[h]);
    }
#pragma unroll
    for (int h = 0; h < H; ++h) {
      gw_part[((size_t)b * H + h) * D + d] = dsh[h] * p[h];
      dpool[h * D + d] = dsh[h] * w[(size_t)h * D + d];
    }
  }
  if (tid < H) gb_part[(size_t)b * H + tid] = ds[head_col(tid, n_front, L)];
  __syncthreads();
  // row pass: da_hi = dpool_h . x_i for all heads from one read of x_i
  for (int i = wave; i < L; i += 4) {
    const float* xr = xb + (size_t)i * D;
    float da[H];
#pragma unroll
    for (int h = 0; h < H; ++h) da[h] = 0.f;
    for (int c = lane * 4; c < D; c += 256) {
      const f32x4_t v = load4(xr + c);
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const f32x4_t dv = *reinterpret_cast<const f32x4_t*>(dpool + h * D + c);
#pragma unroll
        for (int r = 0; r < 4; ++r) da[h] = fmaf(v[r], dv[r], da[h]);
      }
    }
#pragma unroll
    for (int h = 0; h < H; ++h) da[h] = wave_sum(da[h]);
    if (lane == 0) {
#pragma unroll
      for (int h = 0; h < H; ++h) dz[h * Lp + i] = da[h];
    }
  }
  __syncthreads();
  // dz_h = a_h o (da_h - sum_j a_hj da_hj): wave h takes head h
  if (wave < H) {
    const float* ah = av + wave * Lp;
    float* zh = dz + wave * Lp;
    float adot = 0.f;
    for (int i = lane; i < L; i += 64) adot = fmaf(ah[i], zh[i], adot);
    adot = wave_sum(adot);
    for (int i = lane; i < L; i += 64) zh[i] = ah[i] * (zh[i] - adot);
  }
  __syncthreads();
  // gx_i = ds_i u(i) + sum_h (a_hi dpool_h + dz_hi uh_h)
  for (int i = wave; i < L; i += 4) {
    const float* ui = i < ES ? p2 : p1;
    const float s = ds[n_front + i];
    float a[H], zz[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
      a[h] = av[h * Lp + i];
      zz[h] = dz[h * Lp + i];
    }
    float* g = gx + ((size_t)b * L + i) * D;
    for (int c = lane * 4; c < D; c += 256) {
      f32x4_t acc = load4(ui + c) * s;
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const f32x4_t hv = load4(ph + (size_t)h * D + c), dv = *reinterpret_cast<const f32x4_t*>(dpool + h * D + c);
        acc += dv * a[h] + hv * zz[h];
      }
      store4(g + c, acc);
    }
  }
  // column pass 2: gu1 = sum_{i >= ES} ds_i x_i, gu2 = sum_{i < ES} ds_i x_i, guh_h = sum_i dz_hi x_i    (rows in order)
  for (int d = tid; d < D; d += 256) {
    float a1 = 0.f, a2 = 0.f, ah[H];
#pragma unroll
    for (int h = 0; h < H; ++h) ah[h] = 0.f;
    for (int i = 0; i < L; ++i) {
      const float v = xb[(size_t)i * D + d];
      if (i < ES) a2 = fmaf(ds[n_front + i], v, a2);
      else a1 = fmaf(ds[n_front + i], v, a1);
#pragma unroll
      for (int h = 0; h < H; ++h) ah[h] = fmaf(dz[h * Lp + i], v, ah[h]);
    }
    gu1[(size_t)b * D + d] = a1;
    gu2[(size_t)b * D + d] = a2;
#pragma unroll
    for (int h = 0; h < H; ++h) guh[((size_t)b * H + h) * D + d] = ah[h];
  }
}

// the argument contract of both entry points (include/ruart_hip.h)
inline bool scorer_heads_args_ok(int B, int L, int D, int ES, int H, int n_front) {
  return B > 0 && H >= 1 && H <= 4 && n_front >= 0 && n_front <= H && L > 0 && L <= SC_LMAX && ES >= 0 && ES < L && D > 0 && !(D & 3) &&
         scorer_heads_lds_bytes(L, D, H) <= SH_LDS_MAX;
}

}  // namespace

extern "C" int ruart_scorer_fwd(const float* x, const float* u1, const float* u2, const float* uh, const float* w, const float* bna,
                                const unsigned char* mask, float* probs, float* a_out, int B, int L, int D, int ES, int mask_flag,
                                void* stream) {
  RUART_ENTRY();
  if (B <= 0 || L <= 0 || L > SC_LMAX || D <= 0 || (D & 3) || ES < 0 || ES > L || !x || !u1 || !u2 || !uh || !w || !bna || !mask || !probs || !a_out)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(scorer_fwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, u1, u2, uh, w, bna, mask, probs, a_out, L, D, ES,
                     mask_flag, ruart_nan_flag_ptr);
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_scorer_bwd(const float* x, const float* u1, const float* u2, const float* uh, const float* w, const float* probs,
                                const float* a_in, const float* gprobs, float* gx, float* gu1, float* gu2, float* guh, float* gw_part,
                                float* gb_part, int B, int L, int D, int ES, void* stream) {
  RUART_ENTRY();
  if (B <= 0 || L <= 0 || L > SC_LMAX || D <= 0 || (D & 3) || D > 8192 || ES < 0 || ES > L) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(scorer_bwd_kernel, dim3(B), dim3(256), (size_t)D * sizeof(float), (hipStream_t)stream, x, u1, u2, uh, w, probs, a_in,
                     gprobs, gx, gu1, gu2, guh, gw_part, gb_part, L, D, ES);
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_scorer_heads_fwd(const float* x, const float* u1, const float* u2, const float* uh, const float* w, const float* bh,
                                      const unsigned char* mask, float* probs, float* a_out, int B, int L, int D, int ES, int H,
                                      int n_front, int mask_flag, void* stream) {
  RUART_ENTRY();
  if (!scorer_heads_args_ok(B, L, D, ES, H, n_front) || !x || !u1 || !u2 || !uh || !w || !bh || !mask || !probs || !a_out)
    return (int)hipErrorInvalidValue;
  const size_t lds = scorer_heads_lds_bytes(L, D, H);
#define SH_FWD(HH)                                                                                                                   \
  hipLaunchKernelGGL(scorer_heads_fwd_kernel<HH>, dim3(B), dim3(256), lds, (hipStream_t)stream, x, u1, u2, uh, w, bh, mask, probs, a_out, L, \
                     D, ES, n_front, mask_flag, ruart_nan_flag_ptr)
  switch (H) {
    case 1: SH_FWD(1); break;
    case 2: SH_FWD(2); break;
    case 3: SH_FWD(3); break;
    default: SH_FWD(4); break;
  }
#undef SH_FWD
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_scorer_heads_bwd(const float* x, const float* u1, const float* u2, const float* uh, const float* w, const float* probs,
                                      const float* a_in, const float* gprobs, float* gx, float* gu1, float* gu2, float* guh, float* gw_part,
                                      float* gb_part, int B, int L, int D, int ES, int H, int n_front, void* stream) {
  RUART_ENTRY();
  if (!scorer_heads_args_ok(B, L, D, ES, H, n_front) || !x || !u1 || !u2 || !uh || !w || !probs || !a_in || !gprobs || !gx || !gu1 || !gu2 ||
      !guh || !gw_part || !gb_part)
    return (int)hipErrorInvalidValue;
  const size_t lds = scorer_heads_lds_bytes(L, D, H);
#define SH_BWD(HH)                                                                                                                    \
  hipLaunchKernelGGL(scorer_heads_bwd_kernel<HH>, dim3(B), dim3(256), lds, (hipStream_t)stream, x, u1, u2, uh, w, probs, a_in, gprobs, gx, \
                     gu1, gu2, guh, gw_part, gb_part, L, D, ES, n_front)
  switch (H) {
    case 1: SH_BWD(1); break;
    case 2: SH_BWD(2); break;
    case 3: SH_BWD(3); break;
    default: SH_BWD(4); break;
  }
#undef SH_BWD
  RUART_CHECK_LAUNCH();
  return 0;
}
