// Row kernels of the SDNet trunk that are not part of any GEMM, attention or recurrence: the per-item scaling of a packed word matrix
// (variational dropout) and the embedding tables' weight gradient from a host-prepared sort (fp32).
#include "common.h"
#include "ruart_hip.h"

// ------------------------------------------------------------------------------------------------
// out[w][c] = x[w][c] * m[idx[w]][c]: the variational dropout of a PACKED (words, D) matrix whose mask is drawn per (item, feature)
// (layers.row_dropout; Models/Layers.py:23-30 on the reference's padded (items, Lw, D) layout).  One pass instead of torch's gather of the
// mask rows into a (words, D) matrix followed by a multiply (3x the traffic); the backward is the same kernel on the gradient.
// One wave per row, four 16-byte loads in flight per lane; D % 4 == 0, rows 16-byte aligned.
__global__ __launch_bounds__(256) void rows_scale_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ m, int ldm,
                                                         const long long* __restrict__ idx, float* __restrict__ out, int ldo, int rows, int D) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= rows) return;
  const float* xr = x + (size_t)w * ldx;
  const float* mr = m + (size_t)idx[w] * ldm;
  float* orow = out + (size_t)w * ldo;
  for (int c0 = lane * 4; c0 < D; c0 += 4 * 256) {
    f32x4_t a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = min(c0 + u * 256, D - 4);                 // clamped: every load is unconditional
      a[u] = load4(xr + c);
      b[u] = load4(mr + c);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (c0 + u * 256 < D) store4(orow + c0 + u * 256, a[u] * b[u]);
  }
}

extern "C" int ruart_rows_scale(const float* x, int ldx, const float* mask, int ldm, const long long* row_of, float* out, int ldo, int rows,
                                int D, void* stream) {
  RUART_ENTRY();
  if (rows <= 0 || D < 4 || (D & 3) || (ldx & 3) || (ldm & 3) || (ldo & 3) || !x || !mask || !row_of || !out) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(rows_scale_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, ldx, mask, ldm, row_of, out, ldo, rows, D);
  RUART_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------
// Embedding weight gradient from a HOST-prepared sort (Models/SDNet.py:439-493 looks words / POS / entity ids up in
// nn.Embedding tables; torch's backward sorts the ids on the device every step - ~100 launches and ~1 ms for the step's nine
// lookups).  The ids of a batch are known when it is collated, so ruart_amd.batch.BatchIndex sorts them there (numpy, in the
// loader worker): order[] lists the lookup positions grouped by table row, seg_start[s] .. seg_start[s+1] is the slice of
// order[] that hit row seg_row[s].  One workgroup per distinct row adds its gradient rows in that fixed order (no atomics:
// deterministic); rows that were never looked up keep the zero the caller filled gw with.
// A row with very many occurrences (a frequent word; [CLS], [SEP] and the first positions of the trainable encoder's tables: thousands
// per batch) would be one long chain of dependent loads in one workgroup, so the host cuts such rows into sub-segments of <= 64
// occurrences (batch._sort_ids): ruart_embedding_bwd_split sums the sub-segments into a workspace with this kernel (seg_row == NULL:
// segment s -> row s) and then the sub-segment sums of each row into gw with it again (order == NULL: occurrence i is workspace row i).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void embedding_bwd_sorted_kernel(const float* __restrict__ gy, const int* __restrict__ order,
                                                                   const int* __restrict__ seg_start, const int* __restrict__ seg_row,
                                                                   float* __restrict__ gw, int D, int dpad) {
  __shared__ float red[256];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int beg = seg_start[s], end = seg_start[s + 1];
  float* dst = gw + (size_t)(seg_row ? seg_row[s] : s) * D;
  const int G = 256 / dpad;                     // occurrence groups working side by side on narrow tables (dpad = 8..256)
  const int g = tid / dpad, dl = tid % dpad;
  if (G == 1) {
    // wide tables (D > 128; blockIdx.y = chunk of 256 columns): a frequent row - the position table of the trainable encoder has 64
    // rows with ~700 occurrences each - is a chain of dependent loads, so eight occurrences are in flight per lane and the eight partial
    // sums are combined in a fixed order
    const int d = blockIdx.y * 256 + tid;
    if (d >= D) return;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int i = beg;
    for (; i + 7 < end; i += 8) {
      int o[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = order ? order[i + k] : i + k;
#pragma unroll
      for (int k = 0; k < 8; ++k) a[k] += gy[(size_t)o[k] * D + d];
    }
    for (int k = 0; i < end; ++i, ++k) a[k] += gy[(size_t)(order ? order[i] : i) * D + d];
    dst[d] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    return;
  }
  for (int d0 = 0; d0 < D; d0 += dpad) {
    const int d = d0 + dl;
    float acc = 0.f;
    if (d < D)
      for (int i = beg + g; i < end; i += G) acc += gy[(size_t)(order ? order[i] : i) * D + d];
    __syncthreads();
    red[tid] = acc;
    __syncthreads();
    if (g == 0 && d < D) {
      float t = 0.f;
      for (int q = 0; q < G; ++q) t += red[q * dpad + dl];          // fixed order
      dst[d] = t;
    }
  }
}

static void launch_embedding_bwd(const float* gy, const int* order, const int* seg_start, const int* seg_row, int n_seg, int D, float* out,
                                 hipStream_t stream) {
  int dpad = 8;
  while (dpad < D && dpad < 256) dpad <<= 1;
  hipLaunchKernelGGL(embedding_bwd_sorted_kernel, dim3(n_seg, dpad == 256 ? (D + 255) / 256 : 1), dim3(256), 0, stream, gy, order, seg_start,
                     seg_row, out, D, dpad);
}

extern "C" int ruart_embedding_bwd_sorted(const float* grad_out, const int* order, const int* seg_start, const int* seg_row, int n_seg,
                                          int D, float* grad_weight, void* stream) {
  RUART_ENTRY();
  if (n_seg < 0 || D <= 0 || D > 4096 || (n_seg && (!order || !seg_start || !seg_row))) return (int)hipErrorInvalidValue;
  if (n_seg == 0) return 0;
  launch_embedding_bwd(grad_out, order, seg_start, seg_row, n_seg, D, grad_weight, (hipStream_t)stream);
  RUART_CHECK_LAUNCH();
  return 0;
}

extern "C" int ruart_embedding_bwd_split(const float* grad_out, const int* order, const int* sub_start, int n_sub, const int* row_first,
                                         const int* row_id, int n_rows, int D, float* ws, float* grad_weight, void* stream) {
  RUART_ENTRY();
  if (n_sub < 0 || n_rows < 0 || n_rows > n_sub || D <= 0 || D > 4096 || (n_sub && (!order || !sub_start || !row_first || !row_id || !ws)))
    return (int)hipErrorInvalidValue;
  if (n_sub == 0) return 0;
  launch_embedding_bwd(grad_out, order, sub_start, nullptr, n_sub, D, ws, (hipStream_t)stream);          // ws[s] = sum of sub-segment s
  launch_embedding_bwd(ws, nullptr, row_first, row_id, n_rows, D, grad_weight, (hipStream_t)stream);      // gw[row] = its sub-segments, in order
  RUART_CHECK_LAUNCH();
  return 0;
}
