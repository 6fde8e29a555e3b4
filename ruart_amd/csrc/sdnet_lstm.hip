// Persistent LSTM recurrence for the SDNet trunk (fp32).
//
// Reference: Models/Layers.py:166 `self.rnns[i](rnn_input)[0]` -> torch nn.LSTM(batch_first, 1 layer, (bi)directional),
// gate order i, f, g, o, zero initial state, padding NOT masked.  Seven instances, hidden 125
// (Models/SDNet.py:147, 150, 172, 188; Models/Layers.py:489), T up to 100 sequential steps: latency-bound.
//
// The input projection x W_ih^T + b_ih + b_hh for all time steps and both directions is ONE plain GEMM done by the
// caller (xproj).  This file is the sequential part.  In its first form one workgroup per (batch row, direction) keeps its direction's
// W_hh (4h x h, <= 512 x 128 fp32 = 256 KB) entirely in VGPRs - 128 weights per thread - for the whole sequence, the
// running h in LDS (broadcast reads), c in a register.  Two barriers per step, no global traffic for weights.
// Backward (BPTT) is the mirror image with W_hh^T columns in VGPRs; it emits grad_xproj, from which the caller gets
// grad_W_ih, grad_b, grad_x and grad_W_hh with three plain GEMMs.
//
// Three kernel pairs serve ONE entry pair, ruart_lstm_fwd / _bwd (below the streamed pair): the per-row pair that follows, the MFMA
// pair (16 batch rows per workgroup; the default) and, for HP < h <= LSTM_MAX_H, the streamed pair.  The fused cell of the Python-stepped
// route for still larger hidden sizes and the parameter packing come last, each with its entry points.
#include "common.h"
#include "ruart_hip.h"

#define HP 128      // padded hidden size of the resident kernels: up to here W_hh stays in registers for the whole sequence
#define LSTM_MAX_H 256      // largest hidden size of the streamed kernels, and so of ruart_lstm_fwd / _bwd

extern int* ruart_nan_flag_ptr;

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(512) void lstm_fwd_kernel(const float* __restrict__ xproj, const float* __restrict__ w_hh,
                                                       float* __restrict__ y, float* __restrict__ gates, float* __restrict__ cells,
                                                       float* __restrict__ hprev, int T, int h, int ndir, int* __restrict__ nan_flag) {
  __shared__ __attribute__((aligned(16))) float h_s[HP];
  __shared__ float pre_s[4 * HP];
  const int b = blockIdx.x, d = blockIdx.y, g = threadIdx.x;
  const int G = 4 * h;
  const bool row = g < G;
  float w[HP];
  {
    const float* wr = w_hh + ((size_t)d * G + (row ? g : 0)) * h;
#pragma unroll
    for (int j = 0; j < HP; ++j) w[j] = (row && j < h) ? wr[j] : 0.f;
  }
  if (g < HP) h_s[g] = 0.f;
  float c = 0.f;
  const size_t ldx = (size_t)ndir * G, ldy = (size_t)ndir * h;
  const float* xp = xproj + (size_t)b * T * ldx + (size_t)d * G + (row ? g : 0);
  const int t0 = d ? T - 1 : 0, dt = d ? -1 : 1;
  float xnext = row ? xp[(size_t)t0 * ldx] : 0.f;
  __syncthreads();
  bool bad = false;
  for (int s = 0, t = t0; s < T; ++s, t += dt) {
    float pre = xnext;
    if (s + 1 < T && row) xnext = xp[(size_t)(t + dt) * ldx];
    {
      // four independent partial sums: the 128-long dot product is the step's longest dependent chain (one wave per SIMD pair
      // cannot hide a 4-cycle FMA latency 128 times), so it is cut to 32 deep; fixed combination order keeps it deterministic
      float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
      // software-pipelined by hand: the next four 16-byte LDS reads are issued before the 16 FMAs of the current four
      f32x4_t ha[4], hb[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) ha[u] = *reinterpret_cast<const f32x4_t*>(h_s + 4 * u);
#pragma unroll
      for (int jb = 0; jb < HP; jb += 32) {
#pragma unroll
        for (int u = 0; u < 4; ++u) hb[u] = *reinterpret_cast<const f32x4_t*>(h_s + jb + 16 + 4 * u);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = jb + 4 * u;
          p0 = fmaf(w[j], ha[u][0], p0); p1 = fmaf(w[j + 1], ha[u][1], p1);
          p2 = fmaf(w[j + 2], ha[u][2], p2); p3 = fmaf(w[j + 3], ha[u][3], p3);
        }
        if (jb + 32 < HP) {
#pragma unroll
          for (int u = 0; u < 4; ++u) ha[u] = *reinterpret_cast<const f32x4_t*>(h_s + jb + 32 + 4 * u);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = jb + 16 + 4 * u;
          p0 = fmaf(w[j], hb[u][0], p0); p1 = fmaf(w[j + 1], hb[u][1], p1);
          p2 = fmaf(w[j + 2], hb[u][2], p2); p3 = fmaf(w[j + 3], hb[u][3], p3);
        }
      }
      pre += (p0 + p1) + (p2 + p3);
    }
    // every gate row applies its own activation (one v_exp per thread, no divergence: tanh(x) = 2 sigmoid(2x) - 1), so the
    // serial combine below is left with a single tanh per hidden unit
    const size_t o = ((size_t)b * T + t);
    if (row) {
      const bool is_g = (g >= 2 * h) && (g < 3 * h);
      const float sg = 1.0f / (1.0f + __expf(is_g ? -2.0f * pre : -pre));
      const float a = is_g ? 2.0f * sg - 1.0f : sg;
      pre_s[g] = a;
      if (gates) gates[o * ldx + (size_t)d * G + g] = a;
    }
    __syncthreads();
    if (g < h) {
      const float ig = pre_s[g], fg = pre_s[h + g], gg = pre_s[2 * h + g], og = pre_s[3 * h + g];
      c = fg * c + ig * gg;
      const float tc = 2.0f / (1.0f + __expf(-2.0f * c)) - 1.0f;
      const float hh = og * tc;
      if (hprev) hprev[o * ldy + (size_t)d * h + g] = h_s[g];      // h of the previous step of THIS direction (0 at its start)
      h_s[g] = hh;
      y[o * ldy + (size_t)d * h + g] = hh;
      bad |= !(hh == hh);
      if (cells) cells[o * ldy + (size_t)d * h + g] = c;
    }
    __syncthreads();
  }
  if (bad && nan_flag) atomicOr(nan_flag, 1);
}

__global__ __launch_bounds__(512) void lstm_bwd_kernel(const float* __restrict__ grad_y, const float* __restrict__ w_hh,
                                                       const float* __restrict__ gates, const float* __restrict__ cells,
                                                       float* __restrict__ grad_xproj, int T, int h, int ndir) {
  __shared__ __attribute__((aligned(16))) float da_s[4 * HP];
  __shared__ float part_s[4 * HP];
  const int b = blockIdx.x, d = blockIdx.y;
  const int p = threadIdx.x >> 7, j = threadIdx.x & (HP - 1);
  const int G = 4 * h;
  const bool live = j < h;
  float wt[HP];      // wt[r] = W_hh[d][p*h + r][j]
  {
    const float* wc = w_hh + (size_t)d * G * h + (size_t)p * h * h + (live ? j : 0);
#pragma unroll
    for (int r = 0; r < HP; ++r) wt[r] = (live && r < h) ? wc[(size_t)r * h] : 0.f;
  }
  da_s[threadIdx.x] = 0.f;      // pad lanes stay zero for the whole run
  const size_t ldx = (size_t)ndir * G, ldy = (size_t)ndir * h;
  // walk the forward order backwards: dir 0 ran t = 0..T-1, dir 1 ran t = T-1..0
  const int t0 = d ? 0 : T - 1, dt = d ? 1 : -1;
  float dh_rec = 0.f, dc_next = 0.f;
  __syncthreads();
  for (int s = 0, t = t0; s < T; ++s, t += dt) {
    if (p == 0 && live) {
      const size_t o = (size_t)b * T + t;
      const float* gp = gates + o * ldx + (size_t)d * G + j;
      const float ig = gp[0], fg = gp[h], gg = gp[2 * h], og = gp[3 * h];
      const float c = cells[o * ldy + (size_t)d * h + j];
      const float c_prev = (s + 1 < T) ? cells[((size_t)b * T + t + dt) * ldy + (size_t)d * h + j] : 0.f;
      const float dh = grad_y[o * ldy + (size_t)d * h + j] + dh_rec;
      const float tc = tanhf(c);
      const float dc = dc_next + dh * og * (1.f - tc * tc);
      const float da_i = dc * gg * ig * (1.f - ig);
      const float da_f = dc * c_prev * fg * (1.f - fg);
      const float da_g = dc * ig * (1.f - gg * gg);
      const float da_o = dh * tc * og * (1.f - og);
      dc_next = dc * fg;
      da_s[j] = da_i; da_s[HP + j] = da_f; da_s[2 * HP + j] = da_g; da_s[3 * HP + j] = da_o;
      float* gx = grad_xproj + o * ldx + (size_t)d * G + j;
      gx[0] = da_i; gx[h] = da_f; gx[2 * h] = da_g; gx[3 * h] = da_o;
    }
    __syncthreads();
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;      // four partial sums, as in the forward kernel
#pragma unroll
    for (int r = 0; r < HP; r += 4) {
      const f32x4_t dv = *reinterpret_cast<const f32x4_t*>(da_s + p * HP + r);
      a0 = fmaf(wt[r], dv[0], a0); a1 = fmaf(wt[r + 1], dv[1], a1);
      a2 = fmaf(wt[r + 2], dv[2], a2); a3 = fmaf(wt[r + 3], dv[3], a3);
    }
    part_s[threadIdx.x] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (p == 0 && live) dh_rec = (part_s[j] + part_s[HP + j]) + (part_s[2 * HP + j] + part_s[3 * HP + j]);
  }
}

// ---------------------------------------------------------------------------------------------------------
// The same recurrence with 16 batch rows per workgroup on the matrix cores (round 3; default, ruart_lstm_set_variant).
//
// The per-row kernels above pin one CU per (batch row, direction) - 128 workgroups x ~110 us for a (64, 100) layer - and every CU
// they sit on is lost to an encoder GEMM workgroup, which needs a whole CU.  Here a workgroup advances 16
// batch rows at once: the step's recurrent product P (16 x 4h) = h_{t-1} (16 x h) . W_hh^T is an MFMA product with the SDNet
// trunk's split-bf16 arithmetic (hi.hi + hi.lo + lo.hi, fp32 accumulation: ~2^-16 per product, sdnet_gemm.hip), W_hh's hi / lo
// fragments live in VGPRs for the whole sequence (128 per lane, as before), the running h in LDS as the bf16 hi / lo operand
// image (double-buffered: ONE barrier per step).  B x ndir / 16 = 8 workgroups instead of 128.
//
// Ownership.  Wave w, MFMA row m (0..15) stands for hidden unit  unit(w, m) = min(16 w + (m & ~3), h - 4) + (m & 3)  and owns all
// FOUR gate rows of it (the W rows are gathered that way once), so after the MFMAs lane (fr, fq) holds the i, f, g, o
// pre-activations of the four CONSECUTIVE units u0 .. u0 + 3, u0 = min(16 w + 4 fq, h - 4), of batch row fr: the cell update is
// lane-local, c and the previous h stay in registers, nothing is exchanged but the new h.  The clamp makes every lane's four units
// real ones: where 16 w + 4 fq + 3 runs past h (h = 125: the lanes of "units 124..127") the lane recomputes the last four real
// units instead - the same bits as their first owner (same operands, same instruction) - so EVERY lane issues the same full
// 16-byte loads and stores and the loop has no divergent path at all (the first version special-cased the ragged end: ~900
// instructions of exec-mask bookkeeping per step).  Duplicated positions must not be counted twice in a contraction: the W
// entries of a duplicate position are zero.  Batch rows past B are clamped to B - 1 the same way (duplicate, identical stores).
// The backward kernel mirrors it: the lane computes da_i..da_o of its units from the saved gates / cells, writes them to the
// global grad_xproj and to an LDS operand image da (16 x 512 positions, bf16 hi / lo), and after the barrier every wave takes
// dh_{t-1} of ITS 16 positions = da . W_hh[:, units] over all positions from W_hh^T fragments in VGPRs - the result lands in
// the lanes that own those units.
// Memory waits: vmcnt counts loads and stores in one in-order queue, so each step first waits for the NEXT step's operands
// (issued at the top of the step, a whole step ago) and only then issues its own stores - otherwise the wait for the loads would
// also drain the stores (a write latency per step: measured, 1.1 us).
// ---------------------------------------------------------------------------------------------------------
#define LRB 16                 // batch rows per workgroup
#define LHS 272                // forward h image: 128 bf16 per row + 16 bytes pad
#define LDS_DA 1040            // backward da image: 512 bf16 per row + 16 bytes pad
typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));   // 4 consecutive floats at any 4-byte aligned address

__device__ __forceinline__ float sigm_(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.4426950408889634f)); }
__device__ __forceinline__ float tanh_(float x) { return 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -2.8853900817779268f)) - 1.0f; }

__device__ __forceinline__ void split_bf16_(float x, bf16_t& hi, bf16_t& lo) {
  hi = (bf16_t)x;
  lo = (bf16_t)(x - (float)hi);
}
// hidden unit of ownership position (w, m), and whether that position is the unit's first (counted) one
__device__ __forceinline__ int lstm_unit(int w, int m, int h) { return min(16 * w + (m & ~3), h - 4) + (m & 3); }
// Is ownership position q = 16 w + m the one whose weights COUNT in a contraction over positions?  Natural positions (group base
// q & ~3 <= h - 4) always; of the clamped groups only the first one, and there only the units no natural position covers.
__device__ __forceinline__ bool lstm_counted(int q, int h) {
  const int base = q & ~3, b0 = (h - 4) & ~3;
  if (base <= h - 4) return true;
  return base == b0 + 4 && (h - 4 + (q & 3)) > b0 + 3;
}

__global__ __launch_bounds__(512) void lstm_fwd_mfma_kernel(const float* __restrict__ xproj, const float* __restrict__ w_hh,
                                                            float* __restrict__ y, float* __restrict__ gates, float* __restrict__ cells,
                                                            float* __restrict__ hprev, int B, int T, int h, int ndir,
                                                            int* __restrict__ nan_flag) {
  __shared__ __attribute__((aligned(16))) char himg[2][2][LRB * LHS];      // [buffer][hi | lo], k = ownership position 16 w + m
  const int d = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int G = 4 * h;
  // W_hh fragments: first MFMA operand of tile (gate type i, k-step ks) = gate row i*h + unit(w, fr), contraction positions
  // k = 32 ks + 8 fq .. + 7 -> hidden unit of that position; duplicate positions carry zero weights
  bf16x8_t wh[4][4], wl[4][4];
  {
    const int unit = lstm_unit(w, fr, h);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = ks * 32 + fq * 8 + e, kw = k >> 4, km = k & 15;
        const int ku = lstm_unit(kw, km, h);
        const bool counted = lstm_counted(k, h);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float v = counted ? w_hh[((size_t)d * G + (size_t)i * h + unit) * h + ku] : 0.f;
          bf16_t a, b;
          split_bf16_(v, a, b);
          wh[i][ks][e] = a;
          wl[i][ks][e] = b;
        }
      }
  }
  for (int i = tid; i < 2 * 2 * LRB * LHS / 4; i += 512) reinterpret_cast<int*>(&himg[0][0][0])[i] = 0;     // h_0 = 0; pads stay 0
  const int b = min((int)blockIdx.x * LRB + fr, B - 1);
  const int u0 = min(16 * w + 4 * fq, h - 4);          // the lane's units u0 .. u0 + 3 of batch row b
  float c[4] = {0.f, 0.f, 0.f, 0.f}, hp[4] = {0.f, 0.f, 0.f, 0.f};
  const size_t ldx = (size_t)ndir * G, ldy = (size_t)ndir * h;
  const int t0 = d ? T - 1 : 0, dt = d ? -1 : 1;
  const long long sx = (long long)dt * (long long)ldx, sy = (long long)dt * (long long)ldy;      // pointer steps per time step
  const float* xp = xproj + ((size_t)b * T + t0) * ldx + (size_t)d * G + u0;
  const size_t oy = ((size_t)b * T + t0) * ldy + (size_t)d * h + u0, og_ = ((size_t)b * T + t0) * ldx + (size_t)d * G + u0;
  float* yp = y + oy;
  float* cp_ = cells ? cells + oy : nullptr;
  float* hpp = hprev ? hprev + oy : nullptr;
  float* gp = gates ? gates + og_ : nullptr;
  auto load_x = [&](const float* p, f32x4_t (&x)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x4_u v = *reinterpret_cast<const f32x4_u*>(p + (size_t)i * h);
      x[i] = (f32x4_t){v[0], v[1], v[2], v[3]};
    }
  };
  f32x4_t xcur[4], xnext[4];
  load_x(xp, xcur);
#pragma unroll
  for (int i = 0; i < 4; ++i) xnext[i] = xcur[i];
  __syncthreads();
  bool bad = false;
  int cur = 0;
  for (int s = 0; s < T; ++s, cur ^= 1) {
    xp += sx;
    if (s + 1 < T) load_x(xp, xnext);
    bf16x8_t hh[4], hl[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      hh[ks] = *reinterpret_cast<const bf16x8_t*>(&himg[cur][0][fr * LHS + (ks * 32 + fq * 8) * 2]);
      hl[ks] = *reinterpret_cast<const bf16x8_t*>(&himg[cur][1][fr * LHS + (ks * 32 + fq * 8) * 2]);
    }
    f32x4_t acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    // (consecutive MFMAs never touch the same accumulator: a dependent pair stalls for the matrix pipe's latency)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = mfma_16x16x32(wl[i][ks], hh[ks], acc[i]);       // small terms first
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = mfma_16x16x32(wh[i][ks], hl[ks], acc[i]);
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = mfma_16x16x32(wh[i][ks], hh[ks], acc[i]);
    // lane-local cell update of units u0 + r, batch row b
    f32x4_t ga[4], hv, cv, hpv;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float pi = acc[0][r] + xcur[0][r], pf = acc[1][r] + xcur[1][r], pg = acc[2][r] + xcur[2][r], po = acc[3][r] + xcur[3][r];
      // sigmoid(x) = rcp(1 + exp2(-x log2 e)), tanh(x) = 2 sigmoid(2x) - 1 on the raw v_exp_f32 / v_rcp_f32 (1 ulp each): the IEEE
      // divide of 1.0f / (...) is a ten-instruction sequence
      const float ig = sigm_(pi), fg = sigm_(pf), gg = tanh_(pg), og = sigm_(po);
      c[r] = fg * c[r] + ig * gg;
      const float tc = tanh_(c[r]);
      const float hn = og * tc;
      ga[0][r] = ig; ga[1][r] = fg; ga[2][r] = gg; ga[3][r] = og;
      hv[r] = hn;
      cv[r] = c[r];
      hpv[r] = hp[r];
      hp[r] = hn;
      bad |= !(hn == hn);
    }
    {
      // the new h as next step's second operand, at the lane's ownership positions 16 w + 4 fq .. + 3 of row fr
      bf16x4_t vh, vl;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        bf16_t a, bb;
        split_bf16_(hv[r], a, bb);
        vh[r] = a;
        vl[r] = bb;
      }
      *reinterpret_cast<bf16x4_t*>(&himg[cur ^ 1][0][fr * LHS + (16 * w + 4 * fq) * 2]) = vh;
      *reinterpret_cast<bf16x4_t*>(&himg[cur ^ 1][1][fr * LHS + (16 * w + 4 * fq) * 2]) = vl;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // next step's x landed; only the PREVIOUS step's stores were behind it
#pragma unroll
    for (int i = 0; i < 4; ++i) xcur[i] = xnext[i];
    __builtin_amdgcn_sched_barrier(0);
    *reinterpret_cast<f32x4_u*>(yp) = (f32x4_u){hv[0], hv[1], hv[2], hv[3]};
    if (cp_) *reinterpret_cast<f32x4_u*>(cp_) = (f32x4_u){cv[0], cv[1], cv[2], cv[3]};
    if (hpp) *reinterpret_cast<f32x4_u*>(hpp) = (f32x4_u){hpv[0], hpv[1], hpv[2], hpv[3]};
    if (gp) {
#pragma unroll
      for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4_u*>(gp + (size_t)i * h) = (f32x4_u){ga[i][0], ga[i][1], ga[i][2], ga[i][3]};
    }
    yp += sy;
    if (cp_) cp_ += sy;
    if (hpp) hpp += sy;
    if (gp) gp += sx;
    __syncthreads();                                   // the new h image is complete; the old one is dead for every wave
  }
  if (bad && nan_flag) atomicOr(nan_flag, 1);
}

__global__ __launch_bounds__(512) void lstm_bwd_mfma_kernel(const float* __restrict__ grad_y, const float* __restrict__ w_hh,
                                                            const float* __restrict__ gates, const float* __restrict__ cells,
                                                            float* __restrict__ grad_xproj, int B, int T, int h, int ndir) {
  // dh_{t-1} (16 rows x 128 positions) = da_t (16 x 512 positions) . W^T.  Each wave contracts over ITS OWN 64 positions - whose da it
  // has just computed, in registers: the second MFMA operand of k-step j is the lane's own da of gate types 2j and 2j + 1 for its four
  // units, no LDS image of da at all - for ALL 128 output positions (8 tiles), and the eight waves' partial sums meet in LDS: 8 KB
  // written and 8 KB read per wave and step (the first form had every wave read the whole 32 KB da image: 256 KB of LDS reads per step).
  __shared__ __attribute__((aligned(16))) float part[2][8][8][64 * 4];      // [buffer][producer wave][output tile][lane x 4], 128 KB
  const int d = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int G = 4 * h;
  // W_hh^T fragments: first operand of (output tile t8, k-step j) = output position (t8, fr) -> unit(t8, fr); contraction element e of
  // lane group fq = gate type 2j + (e >> 2) of this wave's position 4 fq + (e & 3); duplicate contraction positions carry zero weights
  bf16x8_t wh[8][2], wl[8][2];
  {
#pragma unroll
    for (int t8 = 0; t8 < 8; ++t8) {
      const int unit = lstm_unit(t8, fr, h);
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int type = 2 * j + (e >> 2), m = 4 * fq + (e & 3);
          const int gu = lstm_unit(w, m, h);
          const float v = lstm_counted(16 * w + m, h) ? w_hh[((size_t)d * G + (size_t)type * h + gu) * h + unit] : 0.f;
          bf16_t a, b;
          split_bf16_(v, a, b);
          wh[t8][j][e] = a;
          wl[t8][j][e] = b;
        }
    }
  }
  const int b = min((int)blockIdx.x * LRB + fr, B - 1);
  const int u0 = min(16 * w + 4 * fq, h - 4);
  const size_t ldx = (size_t)ndir * G, ldy = (size_t)ndir * h;
  const int t0 = d ? 0 : T - 1, dt = d ? 1 : -1;       // the forward order walked backwards
  const long long sx = (long long)dt * (long long)ldx, sy = (long long)dt * (long long)ldy;
  float dh_rec[4] = {0.f, 0.f, 0.f, 0.f}, dc_next[4] = {0.f, 0.f, 0.f, 0.f};
  struct StepIn { f32x4_t ig, fg, gg, og, cc, cp, gy; };
  const float* gp = gates + ((size_t)b * T + t0) * ldx + (size_t)d * G + u0;
  const float* cp_ = cells + ((size_t)b * T + t0) * ldy + (size_t)d * h + u0;
  const float* gyp = grad_y + ((size_t)b * T + t0) * ldy + (size_t)d * h + u0;
  float* gx = grad_xproj + ((size_t)b * T + t0) * ldx + (size_t)d * G + u0;
  auto ld = [&](const float* p) -> f32x4_t {
    const f32x4_u v = *reinterpret_cast<const f32x4_u*>(p);
    return (f32x4_t){v[0], v[1], v[2], v[3]};
  };
  // one unconditional 16-byte load per operand, issued ONE STEP AHEAD of their use; `prev`: the forward's previous step exists
  auto load_step = [&](bool prev, StepIn& in) {
    in.ig = ld(gp);
    in.fg = ld(gp + h);
    in.gg = ld(gp + 2 * (size_t)h);
    in.og = ld(gp + 3 * (size_t)h);
    in.cc = ld(cp_);
    in.cp = ld(prev ? cp_ + sy : cp_);                 // (multiplied by 0 below when there is none)
    in.gy = ld(gyp);
  };
  StepIn in, nxt;
  load_step(T > 1, in);
  nxt = in;
  for (int s = 0; s < T; ++s) {
    gp += sx;
    cp_ += sy;
    gyp += sy;
    if (s + 1 < T) load_step(s + 2 < T, nxt);
    const float has_prev = (s + 1 < T) ? 1.f : 0.f;
    f32x4_t da[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float dh = in.gy[r] + dh_rec[r];
      const float tc = tanh_(in.cc[r]);
      const float dc = dc_next[r] + dh * in.og[r] * (1.f - tc * tc);
      da[0][r] = dc * in.gg[r] * in.ig[r] * (1.f - in.ig[r]);
      da[1][r] = dc * (in.cp[r] * has_prev) * in.fg[r] * (1.f - in.fg[r]);
      da[2][r] = dc * in.ig[r] * (1.f - in.gg[r] * in.gg[r]);
      da[3][r] = dh * tc * in.og[r] * (1.f - in.og[r]);
      dc_next[r] = dc * in.fg[r];
    }
    // da as the second MFMA operand of k-step j: [type 2j: units 0..3 | type 2j + 1: units 0..3] of this lane, hi and lo
    bf16x8_t dh_[2], dl_[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        bf16_t a, bb;
        split_bf16_(da[2 * j + (e >> 2)][e & 3], a, bb);
        dh_[j][e] = a;
        dl_[j][e] = bb;
      }
    f32x4_t acc[8];
#pragma unroll
    for (int t8 = 0; t8 < 8; ++t8) acc[t8] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 2; ++j) {                     // (consecutive MFMAs never touch the same accumulator)
#pragma unroll
      for (int t8 = 0; t8 < 8; ++t8) acc[t8] = mfma_16x16x32(wl[t8][j], dh_[j], acc[t8]);       // small terms first
#pragma unroll
      for (int t8 = 0; t8 < 8; ++t8) acc[t8] = mfma_16x16x32(wh[t8][j], dl_[j], acc[t8]);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int t8 = 0; t8 < 8; ++t8) acc[t8] = mfma_16x16x32(wh[t8][j], dh_[j], acc[t8]);
    float* mine = &part[s & 1][w][0][lane * 4];
#pragma unroll
    for (int t8 = 0; t8 < 8; ++t8) *reinterpret_cast<f32x4_t*>(mine + t8 * 256) = acc[t8];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // next step's operands in registers before this step's stores are issued
    in = nxt;
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4_u*>(gx + (size_t)i * h) = (f32x4_u){da[i][0], da[i][1], da[i][2], da[i][3]};
    gx += sx;
    __syncthreads();                                   // (double-buffered: the next step writes the other half)
    // dh of this wave's output tile: the eight waves' partial sums, in wave order
    f32x4_t sum = *reinterpret_cast<const f32x4_t*>(&part[s & 1][0][w][lane * 4]);
#pragma unroll
    for (int pw = 1; pw < 8; ++pw) sum += *reinterpret_cast<const f32x4_t*>(&part[s & 1][pw][w][lane * 4]);
#pragma unroll
    for (int r = 0; r < 4; ++r) dh_rec[r] = sum[r];
  }
}

// ---------------------------------------------------------------------------------------------------------
// The same recurrence for HP < h <= LSTM_MAX_H: the weights are STREAMED.
//
// At h = 256 the bf16 hi / lo image of one direction's W_hh is 4 . 256 . 256 . 4 B = 1 MiB: neither a CU's registers (512 KiB) nor its
// LDS (160 KiB) hold it.  Everything else is lstm_fwd_mfma_kernel's: one workgroup owns 16 batch rows of one direction for the whole
// sequence, lane (fr, fq) of a wave owns all four gates of four consecutive units of batch row fr, the cell update is lane-local, the new
// h goes into the double-buffered bf16 hi / lo LDS image.  There are 256 ownership positions now, in 16 groups of 16: wave w owns groups
// 2 w and 2 w + 1 (lstm_unit / lstm_counted with the group index where the narrow kernels have the wave index).  A preparation kernel
// writes W_hh once per launch, split and already in MFMA fragment order, into the caller's workspace; every step each wave reads ITS slice
// of that image back from L2 with 16-byte loads, 1 KiB per wave instruction, one (k-step, group) chunk - 4 gates x hi / lo = 8 loads -
// ahead of the MFMAs that use it.  The stream does not depend on the step, so the prefetch runs across the step boundary (the last chunk
// of a step prefetches the first chunk of the next).  k-steps past ceil(h / 32), groups past ceil(h / 16) and waves that own no live group
// are skipped with wave-uniform branches: h = 144 streams 5 k-steps, not 8.  No workgroup waits for another one.
// Arithmetic: per k-step lo.hi, hi.lo, then hi.hi into one fp32 accumulator per gate (the resident kernel runs all small terms of a step
// before all hi.hi ones; with a streamed W that would need two passes over the image).
// Backward: dh_{t-1} (16 x 256 positions) = da_t (16 x 1024) . W_hh.  As in lstm_bwd_mfma_kernel every wave contracts over ITS OWN
// positions (2 groups x 4 gate types = 4 k-steps, da straight from its registers) for all live output tiles, streaming the transposed
// image one output tile (8 loads) ahead; a tile's partial sum goes to LDS as soon as its 12 MFMAs are done and the waves' partial sums
// meet there (128 KB, one buffer: two barriers per step).
// Registers (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): lstm_wide_fwd_kernel 214 VGPRs, lstm_wide_bwd_kernel 220 VGPRs; no
// AGPRs, no scratch, 2 waves per SIMD (512 threads); LDS 33 KB / 128 KB.  Measured (profiles/lstm_wide.txt): forward 12.2 us per step at
// h = 256, 6.0 us at h = 144.
// ---------------------------------------------------------------------------------------------------------
#define WLHS 528               // wide forward h image: 256 bf16 per row + 16 bytes pad
#define WSLOTS_CHUNK 512       // 16-byte slots of one streamed chunk: 8 fragments x 64 lanes (8 KiB)

// Forward image, in 16-byte slots: [direction][wave w < KS][k-step ks < KS][group 2 w + gl][gate i][hi | lo][lane], KS = ceil(h / 32).
// Slot (.., lane (fr, fq)) = first MFMA operand of tile (gate row i h + unit(2 w + gl, fr), contraction positions 32 ks + 8 fq .. + 7).
__global__ __launch_bounds__(256) void lstm_wide_prep_fwd_kernel(const float* __restrict__ w_hh, bf16x8_t* __restrict__ img, int h, int KS,
                                                                 int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int lane = idx & 63, p = (idx >> 6) & 1, i = (idx >> 7) & 3, gl = (idx >> 9) & 1;
  int r = idx >> 10;
  const int ks = r % KS;
  r /= KS;
  const int w = r % KS, d = r / KS;
  const int fr = lane & 15, fq = lane >> 4;
  const int unit = lstm_unit(2 * w + gl, fr, h);
  const float* row = w_hh + ((size_t)d * 4 * h + (size_t)i * h + unit) * h;
  bf16x8_t out;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = ks * 32 + fq * 8 + e;
    const float v = lstm_counted(k, h) ? row[lstm_unit(k >> 4, k & 15, h)] : 0.f;
    bf16_t a, b;
    split_bf16_(v, a, b);
    out[e] = p ? b : a;
  }
  img[idx] = out;
}

// Backward image: [direction][producer wave w < KS][output tile t < 2 KS][k-step j = 2 gl + jj][hi | lo][lane].  Slot = first operand of
// (output position (t, fr) -> unit(t, fr); contraction element e of lane group fq = gate type 2 jj + (e >> 2) of position 4 fq + (e & 3) of
// group 2 w + gl); duplicate contraction positions carry zero weights.
__global__ __launch_bounds__(256) void lstm_wide_prep_bwd_kernel(const float* __restrict__ w_hh, bf16x8_t* __restrict__ img, int h, int KS,
                                                                 int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int lane = idx & 63, p = (idx >> 6) & 1, j = (idx >> 7) & 3;
  int r = idx >> 9;
  const int t = r % (2 * KS);
  r /= 2 * KS;
  const int w = r % KS, d = r / KS;
  const int fr = lane & 15, fq = lane >> 4;
  const int unit = lstm_unit(t, fr, h);
  const int g = 2 * w + (j >> 1);
  bf16x8_t out;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int type = 2 * (j & 1) + (e >> 2), m = 4 * fq + (e & 3);
    const int gu = lstm_unit(g, m, h);
    const float v = lstm_counted(16 * g + m, h) ? w_hh[((size_t)d * 4 * h + (size_t)type * h + gu) * h + unit] : 0.f;
    bf16_t a, b;
    split_bf16_(v, a, b);
    out[e] = p ? b : a;
  }
  img[idx] = out;
}

__device__ __forceinline__ bf16x8_t bf16x8_zero_() { return __builtin_bit_cast(bf16x8_t, (f32x4_t){0.f, 0.f, 0.f, 0.f}); }
__device__ __forceinline__ void lstm_wide_loadw(bf16x8_t (&f)[8], const bf16x8_t* p) {
#pragma unroll
  for (int q = 0; q < 8; ++q) f[q] = p[q * 64];
}

__global__ __launch_bounds__(512) void lstm_wide_fwd_kernel(const float* __restrict__ xproj, const bf16x8_t* __restrict__ wimg,
                                                            float* __restrict__ y, float* __restrict__ gates, float* __restrict__ cells,
                                                            float* __restrict__ hprev, int B, int T, int h, int ndir,
                                                            int* __restrict__ nan_flag) {
  __shared__ __attribute__((aligned(16))) char himg[2][2][LRB * WLHS];      // [buffer][hi | lo], k = ownership position, 33 KB
  const int d = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int G = 4 * h, KS = (h + 31) >> 5;
  const bool live0 = 32 * w < h, live1 = 32 * w + 16 < h;      // wave-uniform: does group 2 w / 2 w + 1 hold a real unit?
  for (int i = tid; i < 2 * 2 * LRB * WLHS / 4; i += 512) reinterpret_cast<int*>(&himg[0][0][0])[i] = 0;     // h_0 = 0; pads and dead groups stay 0
  const int b = min((int)blockIdx.x * LRB + fr, B - 1);
  const int uo0 = min(32 * w + 4 * fq, h - 4), uo1 = min(32 * w + 16 + 4 * fq, h - 4);      // first of the lane's four units, per group
  float c[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, hp[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const size_t ldx = (size_t)ndir * G, ldy = (size_t)ndir * h;
  const int t0 = d ? T - 1 : 0, dt = d ? -1 : 1;
  const long long sx = (long long)dt * (long long)ldx, sy = (long long)dt * (long long)ldy;
  const float* xp = xproj + ((size_t)b * T + t0) * ldx + (size_t)d * G;
  const size_t oy = ((size_t)b * T + t0) * ldy + (size_t)d * h, og_ = ((size_t)b * T + t0) * ldx + (size_t)d * G;
  float* yp = y + oy;
  float* cp_ = cells ? cells + oy : nullptr;
  float* hpp = hprev ? hprev + oy : nullptr;
  float* gp = gates ? gates + og_ : nullptr;
  const bf16x8_t* wp = wimg + (size_t)(d * KS + (live0 ? w : 0)) * KS * (2 * WSLOTS_CHUNK) + lane;      // this wave's slice of the image
  auto load_x = [&](const float* p, f32x4_t (&x)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x4_u v = *reinterpret_cast<const f32x4_u*>(p + (size_t)i * h);
      x[i] = (f32x4_t){v[0], v[1], v[2], v[3]};
    }
  };
  // 12 MFMAs of one (k-step, group) chunk; consecutive MFMAs never touch the same accumulator
  auto mma = [&](f32x4_t (&acc)[4], const bf16x8_t (&f)[8], bf16x8_t hh, bf16x8_t hl) {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = mfma_16x16x32(f[2 * i + 1], hh, acc[i]);       // small terms first
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = mfma_16x16x32(f[2 * i], hl, acc[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = mfma_16x16x32(f[2 * i], hh, acc[i]);
  };
  bool bad = false;
  // lane-local cell update of the four units at offset uo (ownership positions pos .. pos + 3 of row fr), and everything it stores
  auto cell = [&](const f32x4_t (&acc)[4], const f32x4_t (&x)[4], float (&cc)[4], float (&hq)[4], int uo, int pos, char* hi_img, char* lo_img) {
    f32x4_t ga[4], hv, cv, hpv;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float pi = acc[0][r] + x[0][r], pf = acc[1][r] + x[1][r], pg = acc[2][r] + x[2][r], po = acc[3][r] + x[3][r];
      const float ig = sigm_(pi), fg = sigm_(pf), gg = tanh_(pg), og = sigm_(po);
      cc[r] = fg * cc[r] + ig * gg;
      const float hn = og * tanh_(cc[r]);
      ga[0][r] = ig; ga[1][r] = fg; ga[2][r] = gg; ga[3][r] = og;
      hv[r] = hn;
      cv[r] = cc[r];
      hpv[r] = hq[r];
      hq[r] = hn;
      bad |= !(hn == hn);
    }
    bf16x4_t vh, vl;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      bf16_t a, bb;
      split_bf16_(hv[r], a, bb);
      vh[r] = a;
      vl[r] = bb;
    }
    *reinterpret_cast<bf16x4_t*>(hi_img + fr * WLHS + pos * 2) = vh;
    *reinterpret_cast<bf16x4_t*>(lo_img + fr * WLHS + pos * 2) = vl;
    *reinterpret_cast<f32x4_u*>(yp + uo) = (f32x4_u){hv[0], hv[1], hv[2], hv[3]};
    if (cp_) *reinterpret_cast<f32x4_u*>(cp_ + uo) = (f32x4_u){cv[0], cv[1], cv[2], cv[3]};
    if (hpp) *reinterpret_cast<f32x4_u*>(hpp + uo) = (f32x4_u){hpv[0], hpv[1], hpv[2], hpv[3]};
    if (gp) {
#pragma unroll
      for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4_u*>(gp + uo + (size_t)i * h) = (f32x4_u){ga[i][0], ga[i][1], ga[i][2], ga[i][3]};
    }
  };
  f32x4_t x0[4], x1[4], xn0[4], xn1[4];
  bf16x8_t wa[8], wb[8];
  load_x(xp + uo0, x0);                               // (dead groups load their clamped, real units: unconditional, never used)
  load_x(xp + uo1, x1);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    xn0[i] = x0[i];
    xn1[i] = x1[i];
    wb[i] = wb[i + 4] = bf16x8_zero_();
  }
  lstm_wide_loadw(wa, wp);                            // chunk (ks 0, group 0) of the first step
  __syncthreads();
  int cur = 0;
  for (int s = 0; s < T; ++s, cur ^= 1) {
    xp += sx;
    if (live0) {
      if (s + 1 < T) {
        load_x(xp + uo0, xn0);
        load_x(xp + uo1, xn1);
      }
      f32x4_t acc0[4], acc1[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc0[i] = acc1[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8_t hh = *reinterpret_cast<const bf16x8_t*>(&himg[cur][0][fr * WLHS + (ks * 32 + fq * 8) * 2]);
        const bf16x8_t hl = *reinterpret_cast<const bf16x8_t*>(&himg[cur][1][fr * WLHS + (ks * 32 + fq * 8) * 2]);
        if (live1) lstm_wide_loadw(wb, wp + (size_t)ks * (2 * WSLOTS_CHUNK) + WSLOTS_CHUNK);
        mma(acc0, wa, hh, hl);
        lstm_wide_loadw(wa, wp + (size_t)(ks + 1 < KS ? ks + 1 : 0) * (2 * WSLOTS_CHUNK));      // wraps into the next step
        if (live1) mma(acc1, wb, hh, hl);
      }
      cell(acc0, x0, c[0], hp[0], uo0, 32 * w + 4 * fq, &himg[cur ^ 1][0][0], &himg[cur ^ 1][1][0]);
      if (live1) cell(acc1, x1, c[1], hp[1], uo1, 32 * w + 16 + 4 * fq, &himg[cur ^ 1][0][0], &himg[cur ^ 1][1][0]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        x0[i] = xn0[i];
        x1[i] = xn1[i];
      }
    }
    yp += sy;
    if (cp_) cp_ += sy;
    if (hpp) hpp += sy;
    if (gp) gp += sx;
    __syncthreads();                                   // the new h image is complete; the old one is dead for every wave
  }
  if (bad && nan_flag) atomicOr(nan_flag, 1);
}

__global__ __launch_bounds__(512) void lstm_wide_bwd_kernel(const float* __restrict__ grad_y, const bf16x8_t* __restrict__ wimg,
                                                            const float* __restrict__ gates, const float* __restrict__ cells,
                                                            float* __restrict__ grad_xproj, int B, int T, int h, int ndir) {
  __shared__ __attribute__((aligned(16))) float part[8][16][64 * 4];      // [producer wave][output tile][lane x 4], 128 KB
  const int d = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int G = 4 * h, KS = (h + 31) >> 5, NG = (h + 15) >> 4;
  const bool live0 = 32 * w < h, live1 = 32 * w + 16 < h;
  const int b = min((int)blockIdx.x * LRB + fr, B - 1);
  const int uo0 = min(32 * w + 4 * fq, h - 4), uo1 = min(32 * w + 16 + 4 * fq, h - 4);
  const size_t ldx = (size_t)ndir * G, ldy = (size_t)ndir * h;
  const int t0 = d ? 0 : T - 1, dt = d ? 1 : -1;       // the forward order walked backwards
  const long long sx = (long long)dt * (long long)ldx, sy = (long long)dt * (long long)ldy;
  float dh_rec[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, dc_next[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  struct StepIn { f32x4_t ig, fg, gg, og, cc, cp, gy; };
  const float* gp = gates + ((size_t)b * T + t0) * ldx + (size_t)d * G;
  const float* cp_ = cells + ((size_t)b * T + t0) * ldy + (size_t)d * h;
  const float* gyp = grad_y + ((size_t)b * T + t0) * ldy + (size_t)d * h;
  float* gx = grad_xproj + ((size_t)b * T + t0) * ldx + (size_t)d * G;
  const bf16x8_t* wp = wimg + (size_t)(d * KS + (live0 ? w : 0)) * (2 * KS) * WSLOTS_CHUNK + lane;      // this wave's slice: 2 KS tile chunks
  auto ld = [&](const float* p) -> f32x4_t {
    const f32x4_u v = *reinterpret_cast<const f32x4_u*>(p);
    return (f32x4_t){v[0], v[1], v[2], v[3]};
  };
  auto load_step = [&](bool prev, int uo, StepIn& in) {
    in.ig = ld(gp + uo);
    in.fg = ld(gp + uo + h);
    in.gg = ld(gp + uo + 2 * (size_t)h);
    in.og = ld(gp + uo + 3 * (size_t)h);
    in.cc = ld(cp_ + uo);
    in.cp = ld(prev ? cp_ + uo + sy : cp_ + uo);       // (multiplied by 0 below when there is none)
    in.gy = ld(gyp + uo);
  };
  // da_i..da_o of the lane's four units of one group -> global grad_xproj and the second MFMA operands of its two k-steps (hi, lo)
  auto step_da = [&](const StepIn& in, float (&dhr)[4], float (&dcn)[4], float has_prev, int uo, bf16x8_t* fh, bf16x8_t* fl) {
    f32x4_t da[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float dh = in.gy[r] + dhr[r];
      const float tc = tanh_(in.cc[r]);
      const float dc = dcn[r] + dh * in.og[r] * (1.f - tc * tc);
      da[0][r] = dc * in.gg[r] * in.ig[r] * (1.f - in.ig[r]);
      da[1][r] = dc * (in.cp[r] * has_prev) * in.fg[r] * (1.f - in.fg[r]);
      da[2][r] = dc * in.ig[r] * (1.f - in.gg[r] * in.gg[r]);
      da[3][r] = dh * tc * in.og[r] * (1.f - in.og[r]);
      dcn[r] = dc * in.fg[r];
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        bf16_t a, bb;
        split_bf16_(da[2 * j + (e >> 2)][e & 3], a, bb);
        fh[j][e] = a;
        fl[j][e] = bb;
      }
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4_u*>(gx + uo + (size_t)i * h) = (f32x4_u){da[i][0], da[i][1], da[i][2], da[i][3]};
  };
  // one output tile: 4 k-steps x 3 products into four independent accumulators, combined in a fixed order
  auto tile = [&](const bf16x8_t (&f)[8], const bf16x8_t (&fh)[4], const bf16x8_t (&fl)[4], float* out) {
    f32x4_t a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = mfma_16x16x32(f[2 * j + 1], fh[j], (f32x4_t){0.f, 0.f, 0.f, 0.f});       // small terms first
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = mfma_16x16x32(f[2 * j], fl[j], a[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = mfma_16x16x32(f[2 * j], fh[j], a[j]);
    *reinterpret_cast<f32x4_t*>(out) = (a[0] + a[1]) + (a[2] + a[3]);
  };
  StepIn in0, in1, n0, n1;
  load_step(T > 1, uo0, in0);
  load_step(T > 1, uo1, in1);
  n0 = in0;
  n1 = in1;
  bf16x8_t wa[8], wb[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) wb[q] = bf16x8_zero_();
  lstm_wide_loadw(wa, wp);                            // output tile 0 of the first step
  for (int s = 0; s < T; ++s) {
    if (live0) {
      const float has_prev = (s + 1 < T) ? 1.f : 0.f;
      bf16x8_t fh[4], fl[4];
      step_da(in0, dh_rec[0], dc_next[0], has_prev, uo0, fh, fl);
      if (live1) {
        step_da(in1, dh_rec[1], dc_next[1], has_prev, uo1, fh + 2, fl + 2);
      } else {
        fh[2] = fh[3] = fl[2] = fl[3] = bf16x8_zero_();
      }
      gp += sx;
      cp_ += sy;
      gyp += sy;
      gx += sx;
      if (s + 1 < T) {                                 // next step's operands, a whole weight stream ahead of their use
        load_step(s + 2 < T, uo0, n0);
        load_step(s + 2 < T, uo1, n1);
      }
      float* mine = &part[w][0][lane * 4];
      for (int tp = 0; tp < KS; ++tp) {
        const bool odd = 2 * tp + 1 < NG;              // (wave-uniform: the last tile of an odd tile count is dead)
        if (odd) lstm_wide_loadw(wb, wp + (size_t)(2 * tp + 1) * WSLOTS_CHUNK);
        tile(wa, fh, fl, mine + (2 * tp) * 256);
        lstm_wide_loadw(wa, wp + (size_t)(tp + 1 < KS ? 2 * tp + 2 : 0) * WSLOTS_CHUNK);      // wraps into the next step
        if (odd) tile(wb, fh, fl, mine + (2 * tp + 1) * 256);
      }
      in0 = n0;
      in1 = n1;
    }
    __syncthreads();
    // dh of this wave's output tiles: the live waves' partial sums, in wave order
    if (live0) {
      f32x4_t s0 = *reinterpret_cast<const f32x4_t*>(&part[0][2 * w][lane * 4]);
      for (int pw = 1; pw < KS; ++pw) s0 += *reinterpret_cast<const f32x4_t*>(&part[pw][2 * w][lane * 4]);
#pragma unroll
      for (int r = 0; r < 4; ++r) dh_rec[0][r] = s0[r];
      if (live1) {
        f32x4_t s1 = *reinterpret_cast<const f32x4_t*>(&part[0][2 * w + 1][lane * 4]);
        for (int pw = 1; pw < KS; ++pw) s1 += *reinterpret_cast<const f32x4_t*>(&part[pw][2 * w + 1][lane * 4]);
#pragma unroll
        for (int r = 0; r < 4; ++r) dh_rec[1][r] = s1[r];
      }
    }
    __syncthreads();                                   // every sum is read before the next step overwrites the buffer
  }
}

// ---------------------------------------------------------------------------------------------------------
// Entry points of the recurrence: one pair for every hidden size 1 .. LSTM_MAX_H.  They choose the kernels: h <= HP the resident ones
// (ruart_lstm_set_variant: MFMA or per-row; h < 4 is always per-row), above it the streamed ones behind their preparation kernel.
// ---------------------------------------------------------------------------------------------------------
static int g_lstm_variant = 1;       // 1: 16 batch rows per workgroup on the matrix cores (default); 0: one workgroup per row, fp32 VALU
extern "C" int ruart_lstm_set_variant(int v) {
  if (v != 0 && v != 1) return (int)hipErrorInvalidValue;
  g_lstm_variant = v;
  return 0;
}

// Workspace of one call, or false for sizes the recurrence does not take.  The resident kernels need none.  The streamed image of either
// pass is ndir x KS x KS chunk pairs of 16 KiB, KS = ceil(h / 32) - 1 MiB per direction at h = 256, 400 KiB at h = 144; the transposed
// (backward) image has the same size, and each call prepares its own, so one workspace serves either call.
static bool lstm_ws_bytes(int h, int ndir, size_t* bytes) {
  if (h < 1 || h > LSTM_MAX_H || ndir < 1 || ndir > 2) return false;
  const size_t KS = (size_t)(h + 31) / 32;
  *bytes = h <= HP ? 0 : (size_t)ndir * KS * KS * 2 * WSLOTS_CHUNK * 16;
  return true;
}

extern "C" int ruart_lstm_ws_bytes(int h, int ndir, size_t* bytes) {
  return bytes && lstm_ws_bytes(h, ndir, bytes) ? 0 : (int)hipErrorInvalidValue;
}

// What both calls check besides their own pointers, before they touch the device: the sizes, and a workspace where one is needed.
static bool lstm_sizes_ok(int B, int T, int h, int ndir, const void* ws, size_t ws_bytes) {
  size_t need;
  return B > 0 && T > 0 && lstm_ws_bytes(h, ndir, &need) && (need == 0 || (ws && ws_bytes >= need));
}

extern "C" int ruart_lstm_fwd(const float* xproj, const float* w_hh, float* y, float* gates, float* cells, float* hprev, int B, int T,
                              int h, int ndir, void* ws, size_t ws_bytes, void* stream) {
  if (!lstm_sizes_ok(B, T, h, ndir, ws, ws_bytes) || !xproj || !w_hh || !y) return (int)hipErrorInvalidValue;
  RUART_ENTRY();
  if (h > HP) {      // the image is prepared in ws by every call: no allocation, no sync
    const int KS = (h + 31) / 32, total = ndir * KS * KS * 2 * WSLOTS_CHUNK;
    hipLaunchKernelGGL(lstm_wide_prep_fwd_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, w_hh, (bf16x8_t*)ws, h, KS, total);
    hipLaunchKernelGGL(lstm_wide_fwd_kernel, dim3((B + LRB - 1) / LRB, ndir), dim3(512), 0, (hipStream_t)stream, xproj, (const bf16x8_t*)ws, y,
                       gates, cells, hprev, B, T, h, ndir, ruart_nan_flag_ptr);
  } else if (g_lstm_variant == 1 && h >= 4) {
    hipLaunchKernelGGL(lstm_fwd_mfma_kernel, dim3((B + LRB - 1) / LRB, ndir), dim3(512), 0, (hipStream_t)stream, xproj, w_hh, y, gates, cells,
                       hprev, B, T, h, ndir, ruart_nan_flag_ptr);
  } else {
    hipLaunchKernelGGL(lstm_fwd_kernel, dim3(B, ndir), dim3(512), 0, (hipStream_t)stream, xproj, w_hh, y, gates, cells, hprev, T, h, ndir,
                       ruart_nan_flag_ptr);
  }
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_lstm_bwd(const float* grad_y, const float* w_hh, const float* gates, const float* cells, float* grad_xproj, int B,
                              int T, int h, int ndir, void* ws, size_t ws_bytes, void* stream) {
  if (!lstm_sizes_ok(B, T, h, ndir, ws, ws_bytes) || !grad_y || !w_hh || !gates || !cells || !grad_xproj) return (int)hipErrorInvalidValue;
  RUART_ENTRY();
  if (h > HP) {
    const int KS = (h + 31) / 32, total = ndir * KS * KS * 2 * WSLOTS_CHUNK;
    hipLaunchKernelGGL(lstm_wide_prep_bwd_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, w_hh, (bf16x8_t*)ws, h, KS, total);
    hipLaunchKernelGGL(lstm_wide_bwd_kernel, dim3((B + LRB - 1) / LRB, ndir), dim3(512), 0, (hipStream_t)stream, grad_y, (const bf16x8_t*)ws, gates,
                       cells, grad_xproj, B, T, h, ndir);
  } else if (g_lstm_variant == 1 && h >= 4) {
    hipLaunchKernelGGL(lstm_bwd_mfma_kernel, dim3((B + LRB - 1) / LRB, ndir), dim3(512), 0, (hipStream_t)stream, grad_y, w_hh, gates, cells,
                       grad_xproj, B, T, h, ndir);
  } else {
    hipLaunchKernelGGL(lstm_bwd_kernel, dim3(B, ndir), dim3(512), 0, (hipStream_t)stream, grad_y, w_hh, gates, cells, grad_xproj, T, h,
                       ndir);
  }
  RUART_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
// Fused LSTM cell for the wide, short `multi2one` LSTM (hidden 300: W_hh does not fit one CU's registers, and the
// sequences are only 1-3 real words long).  The recurrent product h W_hh^T is a plain GEMM per step; this kernel does the
// whole pointwise part of a step in one pass over a ragged, length-sorted batch: rows < n_active are advanced, rows
// >= n_active (items already finished) are carried through unchanged - replacing ~12 elementwise launches forward and ~25
// backward per step.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lstm_cell_fwd_kernel(const float* __restrict__ pre, const float* __restrict__ h_prev,
                                                            const float* __restrict__ c_prev, float* __restrict__ h_out,
                                                            float* __restrict__ c_out, float* __restrict__ acts, int n_active,
                                                            int n_rows, int h) {
  const long long total = (long long)n_rows * h;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += 256LL * gridDim.x) {
    const int r = (int)(e / h), j = (int)(e - (long long)r * h);
    if (r < n_active) {
      const float* p = pre + (size_t)r * 4 * h + j;
      const float ig = 1.0f / (1.0f + __expf(-p[0])), fg = 1.0f / (1.0f + __expf(-p[h]));
      const float gg = 2.0f / (1.0f + __expf(-2.0f * p[2 * h])) - 1.0f, og = 1.0f / (1.0f + __expf(-p[3 * h]));
      const float c = fg * c_prev[e] + ig * gg;
      const float tc = 2.0f / (1.0f + __expf(-2.0f * c)) - 1.0f;
      c_out[e] = c;
      h_out[e] = og * tc;
      float* a = acts + (size_t)r * 4 * h + j;
      a[0] = ig; a[h] = fg; a[2 * h] = gg; a[3 * h] = og;
    } else {
      c_out[e] = c_prev[e];
      h_out[e] = h_prev[e];
    }
  }
}

__global__ __launch_bounds__(256) void lstm_cell_bwd_kernel(const float* __restrict__ gh, const float* __restrict__ gc,
                                                            const float* __restrict__ acts, const float* __restrict__ c_prev,
                                                            const float* __restrict__ c_out, float* __restrict__ g_pre,
                                                            float* __restrict__ g_hprev, float* __restrict__ g_cprev, int n_active,
                                                            int n_rows, int h) {
  const long long total = (long long)n_rows * h;
  for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += 256LL * gridDim.x) {
    const int r = (int)(e / h), j = (int)(e - (long long)r * h);
    const float dh = gh ? gh[e] : 0.f, dcn = gc ? gc[e] : 0.f;
    if (r < n_active) {
      const float* a = acts + (size_t)r * 4 * h + j;
      const float ig = a[0], fg = a[h], gg = a[2 * h], og = a[3 * h];
      const float c = c_out[e];
      const float tc = 2.0f / (1.0f + __expf(-2.0f * c)) - 1.0f;
      const float dc = dcn + dh * og * (1.f - tc * tc);
      float* g = g_pre + (size_t)r * 4 * h + j;
      g[0] = dc * gg * ig * (1.f - ig);
      g[h] = dc * c_prev[e] * fg * (1.f - fg);
      g[2 * h] = dc * ig * (1.f - gg * gg);
      g[3 * h] = dh * tc * og * (1.f - og);
      g_cprev[e] = dc * fg;
      g_hprev[e] = 0.f;              // the recurrent path of h_prev goes through the GEMM (autograd adds it)
    } else {
      g_cprev[e] = dcn;
      g_hprev[e] = dh;
    }
  }
}

extern "C" int ruart_lstm_cell_fwd(const float* pre, const float* h_prev, const float* c_prev, float* h_out, float* c_out,
                                   float* acts, int n_active, int n_rows, int h, void* stream) {
  RUART_ENTRY();
  if (n_rows <= 0 || h <= 0 || n_active < 0 || n_active > n_rows) return (int)hipErrorInvalidValue;
  const long long total = (long long)n_rows * h;
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, pre, h_prev, c_prev, h_out, c_out, acts,
                     n_active, n_rows, h);
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_lstm_cell_bwd(const float* grad_h, const float* grad_c, const float* acts, const float* c_prev,
                                   const float* c_out, float* grad_pre, float* grad_h_prev, float* grad_c_prev, int n_active,
                                   int n_rows, int h, void* stream) {
  RUART_ENTRY();
  if (n_rows <= 0 || h <= 0 || n_active < 0 || n_active > n_rows) return (int)hipErrorInvalidValue;
  const long long total = (long long)n_rows * h;
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, grad_h, grad_c, acts, c_prev, c_out,
                     grad_pre, grad_h_prev, grad_c_prev, n_active, n_rows, h);
  RUART_CHECK_LAUNCH();
  return 0;
}

// The operands one bidirectional nn.LSTM layer's kernels take, assembled from its eight parameter tensors in ONE launch (torch: two
// cats, two adds and a stack - five launches per layer and step, 55 of a step's ~900):
//   w (2 G, K) = [w_ih ; w_ih_r],  b (2 G) = [b_ih + b_hh ; b_ih_r + b_hh_r],  whh (2, G, h) = [w_hh , w_hh_r]      (G = 4 h)
__global__ void lstm_pack_params_kernel(const float* __restrict__ w_ih, const float* __restrict__ w_ih_r, const float* __restrict__ b_ih,
                                        const float* __restrict__ b_hh, const float* __restrict__ b_ih_r, const float* __restrict__ b_hh_r,
                                        const float* __restrict__ w_hh, const float* __restrict__ w_hh_r, float* __restrict__ w,
                                        float* __restrict__ b, float* __restrict__ whh, long long n_w, long long n_hh, int G) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * n_w + 2 * n_hh + 2 * G; i += stride) {
    if (i < n_w) {
      w[i] = w_ih[i];
    } else if (i < 2 * n_w) {
      w[i] = w_ih_r[i - n_w];
    } else if (i < 2 * n_w + n_hh) {
      whh[i - 2 * n_w] = w_hh[i - 2 * n_w];
    } else if (i < 2 * n_w + 2 * n_hh) {
      whh[i - 2 * n_w] = w_hh_r[i - 2 * n_w - n_hh];
    } else {
      const int j = (int)(i - 2 * n_w - 2 * n_hh);
      b[j] = j < G ? b_ih[j] + b_hh[j] : b_ih_r[j - G] + b_hh_r[j - G];
    }
  }
}

extern "C" int ruart_lstm_pack_params(const float* w_ih, const float* w_ih_r, const float* b_ih, const float* b_hh, const float* b_ih_r,
                                      const float* b_hh_r, const float* w_hh, const float* w_hh_r, float* w, float* b, float* whh, int G,
                                      int K, int h, void* stream) {
  RUART_ENTRY();
  if (G <= 0 || K <= 0 || h <= 0 || !w_ih || !w_ih_r || !b_ih || !b_hh || !b_ih_r || !b_hh_r || !w_hh || !w_hh_r || !w || !b || !whh)
    return (int)hipErrorInvalidValue;
  const long long n_w = (long long)G * K, n_hh = (long long)G * h;
  const long long total = 2 * n_w + 2 * n_hh + 2 * G;
  const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL(lstm_pack_params_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w_ih, w_ih_r, b_ih, b_hh, b_ih_r, b_hh_r, w_hh,
                     w_hh_r, w, b, whh, n_w, n_hh, G);
  RUART_CHECK_LAUNCH();
  return 0;
}
