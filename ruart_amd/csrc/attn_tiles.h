// Device helpers shared by the trunk attention kernels: sdnet_attention.hip (key sets of up to 384, the whole key / value panel in LDS)
// and sdnet_attention_wide.hip (385 .. 1024 keys, the panels walked in key blocks).  Moved here unchanged from sdnet_attention.hip, whose
// head comment explains the LDS strides; everything is __forceinline__, so each file's kernels keep their own code.
#pragma once
#include "common.h"

#define CH 64          // chunk of the contraction / output dimension staged per pass
#define LDA_ 66        // A-type stride for a 64-wide chunk   (66 % 32 == 2)
#define LDB_ 80        // B-type stride for a 64-wide chunk   (80 % 32 == 16)

__device__ __forceinline__ f32x4_t mma16(const float* As, int lda, const float* Bs, int sbk, int sbj, int Kc, f32x4_t acc) {
  const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
  for (int kk = 0; kk < Kc; kk += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(As[r * lda + kk + q], Bs[(kk + q) * sbk + r * sbj], acc, 0, 0, 0);
  return acc;
}

// Activation folded into the staging of the projected operands (Layers.py:228-231): a = ReLU(p1) * diag, k = ReLU(p2).
// diag_len: 0 = none, 1 = one scalar (do_similarity), otherwise a per-column vector of that length.
struct Act {
  int relu;
  const float* diag;
  int diag_len;
  __device__ __forceinline__ float operator()(float v, int col) const {
    if (relu) v = fmaxf(v, 0.f);
    if (diag_len == 1) v *= diag[0];
    else if (diag_len > 1) v *= diag[col];
    return v;
  }
};
__device__ __forceinline__ Act no_act() { return Act{0, nullptr, 0}; }

// stage rows [r0, r0+nr) x cols [c0, c0+CH) of a row-major (rows x cols, ld) matrix into dst[nr_pad][ldd], zero-filled.
// Sixteen independent loads in flight per thread before the first LDS store.  Every load is UNCONDITIONAL - out-of-range elements
// read a clamped (valid) address and are zeroed by a select when they are stored.  Rounds 1-3 wrote `in_range ? src[..] : 0`: hipcc
// branches around such a load and waits vmcnt(0) behind it (cdna_hip_programming.md, projection GEMM item 4c), so the "sixteen in
// flight" were sixteen dependent L2 round trips and the three attention kernels ran at 0.85 TB/s.
template <int U>
__device__ __forceinline__ void stage_u(float* dst, int ldd, int nr_pad, const float* src, int ld, int r0, int rows, int c0, int cols, Act act) {
  const int total = nr_pad * CH;
  for (int e0 = threadIdx.x; e0 < total; e0 += U * blockDim.x) {
    float v[U], dv[U];
    unsigned ok = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = e0 + u * blockDim.x;
      const int r = e / CH, c = e % CH;
      const int gr = r0 + r, gc = c0 + c;
      if (e < total && gr < rows && gc < cols) ok |= 1u << u;
      v[u] = src[(size_t)min(gr, rows - 1) * ld + min(gc, cols - 1)];
    }
    if (act.diag_len > 1) {                      // (wave-uniform: one branch around the group, not one per load)
#pragma unroll
      for (int u = 0; u < U; ++u) dv[u] = act.diag[min(c0 + (e0 + u * (int)blockDim.x) % CH, cols - 1)];
    } else {
      const float d1 = act.diag_len == 1 ? act.diag[0] : 1.f;
#pragma unroll
      for (int u = 0; u < U; ++u) dv[u] = d1;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = e0 + u * blockDim.x;
      float x = v[u];
      if (act.relu) x = fmaxf(x, 0.f);
      x *= dv[u];
      if (e < total) dst[(e / CH) * ldd + (e % CH)] = ((ok >> u) & 1u) ? x : 0.f;
    }
  }
}
// the loads in flight per thread follow the tile: a 16-row tile is 4 elements per thread (the trainable encoder's short windows call
// these kernels with 16-row key panels too - sixteen clamped loads each would be 4x the traffic), a 64-row panel 16
__device__ __forceinline__ void stage(float* dst, int ldd, int nr_pad, const float* src, int ld, int r0, int rows, int c0, int cols,
                                      Act act = Act{0, nullptr, 0}) {
  if (nr_pad <= 16) stage_u<4>(dst, ldd, nr_pad, src, ld, r0, rows, c0, cols, act);
  else if (nr_pad <= 32) stage_u<8>(dst, ldd, nr_pad, src, ld, r0, rows, c0, cols, act);
  else stage_u<16>(dst, ldd, nr_pad, src, ld, r0, rows, c0, cols, act);
}

__device__ __forceinline__ int lds_probs_stride(int L2p) { return ((L2p + 31) / 32) * 32 + 2; }

// A register-prefetched operand chunk (sdnet_attention.hip, "Round 5"): loaded right after the previous chunk's registers have gone to
// LDS, so that the loads fly under that chunk's MFMAs; every load unconditional, validity bits applied at the LDS store.
template <int U, bool DIAG = false>
struct Panel {
  float v[U];
  float dv[DIAG ? U : 1];
  unsigned ok;
  // rows [r0, r0 + nr_pad) x cols [c0, c0 + CH) of a row-major (rows x cols, ld) matrix; nr_pad * CH <= U * 256
  __device__ __forceinline__ void load(const float* __restrict__ src, int ld, int nr_pad, int r0, int rows, int c0, int cols,
                                       const float* __restrict__ diag = nullptr, int diag_len = 0) {
    ok = 0;
    const int total = nr_pad * CH;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = (int)threadIdx.x + u * 256;
      const int r = e / CH, c = e % CH;
      const int gr = r0 + r, gc = c0 + c;
      if (e < total && gr < rows && gc < cols) ok |= 1u << u;
      v[u] = src[(size_t)min(gr, rows - 1) * ld + min(gc, cols - 1)];
      if (DIAG) dv[u] = diag_len > 1 ? diag[min(gc, cols - 1)] : (diag_len == 1 ? diag[0] : 1.f);
    }
  }
  __device__ __forceinline__ void store(float* dst, int ldd, int nr_pad, int relu) const {
    const int total = nr_pad * CH;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = (int)threadIdx.x + u * 256;
      float x = v[u];
      if (relu) x = fmaxf(x, 0.f);
      x *= DIAG ? dv[u] : 1.f;
      if (e < total) dst[(e / CH) * ldd + (e % CH)] = ((ok >> u) & 1u) ? x : 0.f;
    }
  }
};

// backward B with prefetch: the (n0, r0) chunk pairs of a product in one flattened walk, the next pair's operands in flight under this
// pair's MFMAs.  X^T tile: 16 source columns x 64 rows (4 elements per thread, optionally times `xmul`), Y chunk: 64 x 64 (16 per thread).
struct PanelT16 {
  float v[4], m[4];
  unsigned ok;
  __device__ __forceinline__ void load(const float* __restrict__ src, int ld, int r0, int rows, int c0, int cols, const float* __restrict__ mul) {
    ok = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = (int)threadIdx.x + u * 256;
      const int c = e & 15, r = e >> 4;
      const int gr = r0 + r, gc = c0 + c;
      if (gr < rows && gc < cols) ok |= 1u << u;
      const size_t at = (size_t)min(gr, rows - 1) * ld + min(gc, cols - 1);
      v[u] = src[at];
      m[u] = mul ? mul[at] : 1.f;
    }
  }
  __device__ __forceinline__ void store(float* dst, int ldd) const {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = (int)threadIdx.x + u * 256;
      dst[(e & 15) * ldd + (e >> 4)] = ((ok >> u) & 1u) ? v[u] * m[u] : 0.f;
    }
  }
};

// per (batch, 16 key rows): C[16 j][N] = X^T . Y with X (L1 x L2) in {dS, P}, Y (L1 x N) in {a, gO}; no limit on L2
__device__ __forceinline__ void tn_product_pf(const float* X, int L1, int L2, int j0, const float* Y, int N, float* C, float* xt_s,
                                              float* y_s, Act yact, const float* out_gate, const float* xmul) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nr = (L1 + CH - 1) / CH, nn = (N + CH - 1) / CH, steps = nr * nn;
  PanelT16 px;
  Panel<16, true> py;
  px.load(X, L2, 0, L1, j0, L2, xmul);
  py.load(Y, N, CH, 0, L1, 0, N, yact.diag, yact.diag_len);
  f32x4_t o = {0.f, 0.f, 0.f, 0.f};
  int ri = 0, ni = 0;
  for (int s = 0; s < steps; ++s) {
    const int r0 = ri * CH, n0 = ni * CH;
    __syncthreads();
    px.store(xt_s, LDA_);
    py.store(y_s, LDB_, CH, yact.relu);
    int rn = ri + 1, nx = ni;
    if (rn == nr) { rn = 0; nx = ni + 1; }
    if (nx == nn) { rn = 0; nx = 0; }              // (past the end: a clamped re-read of the first pair, never stored)
    px.load(X, L2, rn * CH, L1, j0, L2, xmul);
    py.load(Y, N, CH, rn * CH, L1, nx * CH, N, yact.diag, yact.diag_len);
    __syncthreads();
    const int kc = min(CH, (L1 - r0 + 3) & ~3);
    o = mma16(xt_s, LDA_, y_s + wave * 16, LDB_, 1, kc, o);
    if (ri == nr - 1) {                              // the chunk column is complete
      const int n = n0 + wave * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + (lane >> 4) * 4 + r;
        if (j < L2 && n < N) {
          const size_t at = (size_t)j * N + n;
          C[at] = (out_gate && out_gate[at] <= 0.f) ? 0.f : o[r];
        }
      }
      o = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    }
    ri = rn;
    ni = nx;
  }
}
