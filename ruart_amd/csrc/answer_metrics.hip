// Answer-string metrics: batched unit-cost Levenshtein distance over pairs of code-point strings.
//
//   ruart_edit_distance_pairs    Utils/eval_func.py:13-24 (the distance inside the ANLS per-pair score) and the string equality of
//                                :62-68 (the VQA accuracy count), for every (candidate, answer) pair of a batch in one launch.
//
// One wavefront per pair.  String a lies along the lanes in blocks of 64 columns, string b along the rows; the table is swept by
// anti-diagonals: at step t lane l holds row i = t - l + 1 of its column, so that the cell above is the lane's own last value, the
// cell to the left is the left neighbour's last value (__shfl_up) and the diagonal cell is the `left` of the step before.  The last
// column of a block is the next block's left boundary and goes through LDS (written by lane 63 at step i + 62, read by lane 0 of the
// next block at step i - 1 of its own sweep: the block sweeps are sequential, so the buffer is reused in place).  Everything a lane
// keeps is a scalar register; the only arrays are the wave's two LDS rows (b's code points and the boundary column).
//
// Memory safety does not depend on the index arrays' contents: each pair's two string indices are checked against n_str, its four
// offsets against [0, n_chars] and each other, its two lengths against RUART_EDIT_MAX_LEN, before anything is read through them; a
// pair that fails gets dist = -1, equal = 0.
#include "common.h"
#include "ruart_hip.h"

namespace {

constexpr int kCap = RUART_EDIT_MAX_LEN;
constexpr int kWaves = 4;

__global__ __launch_bounds__(kWaves * 64) void edit_distance_pairs_kernel(const int* __restrict__ chars, int n_chars,
                                                                            const int* __restrict__ str_off, int n_str,
                                                                            const int* __restrict__ pair_a, const int* __restrict__ pair_b,
                                                                            int n_pairs, int* __restrict__ dist, int* __restrict__ equal) {
  __shared__ int b_chars[kWaves][kCap];
  __shared__ int boundary[kWaves][kCap + 1];          // boundary[i] = D[i][64 k] of the block before (rows 0 .. lb)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p = blockIdx.x * kWaves + wave;
  if (p >= n_pairs) return;                             // (wave-uniform; no workgroup barrier below)
  const int ia = pair_a[p], ib = pair_b[p];
  bool ok = ia >= 0 && ia < n_str && ib >= 0 && ib < n_str;
  int a0 = 0, a1 = 0, b0 = 0, b1 = 0;
  if (ok) {
    a0 = str_off[ia], a1 = str_off[ia + 1], b0 = str_off[ib], b1 = str_off[ib + 1];
    ok = a0 >= 0 && a0 <= a1 && a1 <= n_chars && a1 - a0 <= kCap && b0 >= 0 && b0 <= b1 && b1 <= n_chars && b1 - b0 <= kCap;
  }
  if (!ok) {
    if (lane == 0) dist[p] = -1, equal[p] = 0;
    return;
  }
  const int la = a1 - a0, lb = b1 - b0;
  if (la == 0 || lb == 0) {
    if (lane == 0) dist[p] = la + lb, equal[p] = (la + lb) == 0;
    return;
  }
  // volatile: the lanes of the wave hand values to each other through these rows in program order (no workgroup barrier is involved:
  // the waves of a workgroup work on different pairs with different trip counts)
  volatile int* bc = b_chars[wave];
  volatile int* bound = boundary[wave];
  for (int i = lane; i < lb; i += 64) bc[i] = chars[b0 + i];
  for (int i = lane; i <= lb; i += 64) bound[i] = i;   // left boundary of the first block: D[i][0] = i
  __builtin_amdgcn_wave_barrier();
  int result = 0;
  for (int col0 = 0; col0 < la; col0 += 64) {
    const int ncols = min(64, la - col0);
    const int j = col0 + lane + 1;                      // this lane's column (1-based); lanes >= ncols compute cells nobody reads
    const int ca = lane < ncols ? chars[a0 + col0 + lane] : -1;
    int cur = j;                                        // D[0][j]
    int diag = j - 1;                                   // D[0][j - 1]
    const int steps = lb + ncols - 1;
    for (int t = 0; t < steps; ++t) {
      const int i = t - lane + 1;                       // this lane's row at this step (1-based)
      const bool active = i >= 1 && i <= lb;
      const int ic = active ? i : 1;                    // (an index inside both LDS rows for the idle lanes)
      int left = __shfl_up(cur, 1, 64);
      if (lane == 0) left = bound[ic];
      const int cb = bc[ic - 1];
      const int v = min(min(cur, left) + 1, diag + (ca != cb));
      if (active) {
        cur = v;
        diag = left;
        if (lane == 63) bound[i] = v;                   // the next block's left boundary
      }
    }
    result = __shfl(cur, ncols - 1, 64);                // D[lb][col0 + ncols]: the answer once this is the last block
  }
  if (lane == 0) dist[p] = result, equal[p] = result == 0;
}

}  // namespace

extern "C" int ruart_edit_distance_pairs(const int32_t* chars, int n_chars, const int32_t* str_off, int n_str, const int32_t* pair_a,
                                         const int32_t* pair_b, int n_pairs, int32_t* dist, int32_t* equal, void* stream) {
  RUART_ENTRY();
  if (!chars || !str_off || !pair_a || !pair_b || !dist || !equal) return (int)hipErrorInvalidValue;
  if (n_chars < 0 || n_str < 0 || n_pairs < 0) return (int)hipErrorInvalidValue;
  if (n_pairs == 0) return 0;
  if (n_str == 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(edit_distance_pairs_kernel, dim3(ceil_div(n_pairs, kWaves)), dim3(kWaves * 64), 0, (hipStream_t)stream, chars,
                     n_chars, str_off, n_str, pair_a, pair_b, n_pairs, dist, equal);
  RUART_CHECK_LAUNCH();
  return 0;
}
