// lotus-hip: the context part of the stem of SimplePolicyPTV3Concat (genrobo3d/models/simple_policy_ptv3.py:457-461 repeats one
// context vector per cloud over the cloud's points and concatenates it to pc_fts; PointTransformerV3/model.py:844-853 is the 5^3
// SubMConv3d that reads the result).  The convolution is linear in its input columns and the context columns are constant over a
// cloud, so with P[b][t] = W_ctx[:, t, :] ctx_b ([B][T][C], one small dense product):
//   conv(W, [pc | ctx_b(i)])_i = conv(W_pc, pc)_i + sum over the taps t with nbr[t][i] >= 0 of P[b(i)][t]
// (a neighbour is always in the same cloud: the batch index is part of the voxel key).  Only the SIGN of a table entry is read.
//   forward:   y_i = add_i + sum_{t ascending, present} P[b(i)][t]
//   backward:  dP[b][t] = sum_{i in cloud b, present} dy_i
// fp32 only (no bf16-storage twin).  Both grids run over (cloud, row chunk): a block never straddles two clouds, and the cloud's
// P slice (forward) or dP partial (backward) sits in LDS, T x C floats.  The table is read tap by tap with one thread per (row,
// presence word) — for a fixed tap the rows of a tile are consecutive ints — into a two-word presence mask per row in LDS; the sums
// then run with consecutive lanes on consecutive column quads of a row (row-contiguous loads and stores).  No atomics: forward adds
// the taps in ascending order, backward adds rows in ascending order per chunk and lotus_reduce_parts merges the CT_SPLITS chunk
// partials of a cloud in fixed order, so reruns are bit-identical and a tap present nowhere in a cloud gets an exact 0.
#include "common.h"

namespace LOTUS_NS {

#define CT_ROWS 128      // rows per chunk, forward (the grid is cdiv(n, CT_ROWS) x B; chunks past a cloud's end return at once):
                         // 256 threads = 128 rows x 2 presence words, and 512 blocks at 16 x 4096 rows
#define CT_SPLITS 32     // row chunks per cloud, backward (fixed: the workspace is CT_SPLITS B T C floats)
#define CT_BTILE 512     // rows per mask tile, backward
#define CT_MAX_TC 32768  // T x C floats of LDS: 128 KB (+ 8 KB of masks in backward) of the 160 KB of a CU
#define CT_TMAX 128      // two 64-bit presence words per row

typedef unsigned long long ct_u64;

// presence word w of `row`: bit t - 64 w set iff nbr[t][row] >= 0, t in [64 w, min(T, 64 w + 64))
__device__ __forceinline__ ct_u64 ct_word_mask(const int* __restrict__ nbr, int n, int T, int row, int w) {
  ct_u64 m = 0;
  const int t0 = 64 * w, t1 = T < t0 + 64 ? T : t0 + 64;
  const int* p = nbr + (long)t0 * n + row;
#pragma unroll 8
  for (int t = t0; t < t1; ++t, p += n) m |= (ct_u64)(*p >= 0) << (t - t0);
  return m;
}

__device__ __forceinline__ void ct_add4(float4& a, const float4 v) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }

__global__ __launch_bounds__(256) void ctx_taps_fwd_kernel(const float* __restrict__ P, const int* __restrict__ nbr,
                                                           const int* __restrict__ off, const float* __restrict__ add,
                                                           float* __restrict__ y, int n, int T, int C) {
  LOTUS_T_PRIO();
  extern __shared__ float4 ct_p[];  // P[b]: [T][C / 4] float4
  __shared__ ct_u64 msk[2][CT_ROWS];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n0 = max(off[b], 0), n1 = min(off[b + 1], n);
  const long pl = (long)n0 + (long)blockIdx.x * CT_ROWS;
  if (pl >= n1) return;  // (uniform over the block)
  const int p0 = (int)pl, p1 = min(p0 + CT_ROWS, n1);
  const int c4 = C / 4, tc4 = T * c4;
  const float* Pb = P + (long)b * T * C;
  for (int i = tid; i < tc4; i += 256) ct_p[i] = ld4q(Pb, i);
  {
    const int w = tid / CT_ROWS, r = tid % CT_ROWS;
    msk[w][r] = p0 + r < p1 ? ct_word_mask(nbr, n, T, p0 + r, w) : 0;
  }
  __syncthreads();
  const int items = (p1 - p0) * c4;
  for (int e = tid; e < items; e += 256) {
    const int r = e / c4, q = e - r * c4;
    const long row = p0 + r;
    float4 a = add ? ld4q(add + row * C, q) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (ct_u64 m = msk[0][r]; m; m &= m - 1) ct_add4(a, ct_p[__builtin_ctzll(m) * c4 + q]);
    for (ct_u64 m = msk[1][r]; m; m &= m - 1) ct_add4(a, ct_p[(64 + __builtin_ctzll(m)) * c4 + q]);
    st4q(y + row * C, q, a);
  }
}

// chunk s of cloud b -> part[s][b][T][C]
__global__ __launch_bounds__(256) void ctx_taps_bwd_kernel(const float* __restrict__ dy, const int* __restrict__ nbr,
                                                           const int* __restrict__ off, float* __restrict__ part, int B, int n,
                                                           int T, int C) {
  LOTUS_T_PRIO();
  extern __shared__ float4 ct_acc[];  // [T][C / 4] float4 sums, then [2][CT_BTILE] presence words
  const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int c4 = C / 4, tc4 = T * c4;
  ct_u64* msk = reinterpret_cast<ct_u64*>(ct_acc + tc4);
  const int n0 = max(off[b], 0), n1 = max(min(off[b + 1], n), n0), nn = n1 - n0;
  const int p0 = n0 + (int)((long)nn * s / CT_SPLITS), p1 = n0 + (int)((long)nn * (s + 1) / CT_SPLITS);
  // element e of the sums belongs to thread e % 256 throughout: no barrier around the sums themselves
  for (int e = tid; e < tc4; e += 256) ct_acc[e] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int r0 = p0; r0 < p1; r0 += CT_BTILE) {
    __syncthreads();
    for (int i = tid; i < 2 * CT_BTILE; i += 256) {
      const int w = i / CT_BTILE, rr = i % CT_BTILE;
      if (r0 + rr < p1) msk[i] = ct_word_mask(nbr, n, T, r0 + rr, w);
    }
    __syncthreads();
    const int rows = min(CT_BTILE, p1 - r0);
    for (int e = tid; e < tc4; e += 256) {
      const int t = e / c4, q = e - t * c4;
      const ct_u64 bit = (ct_u64)1 << (t & 63);
      const ct_u64* mw = msk + (t >> 6) * CT_BTILE;
      const float* d = dy + (long)r0 * C + 4 * q;
      float4 a = ct_acc[e];
      // every row of the tile is loaded (L1 / L2 hits shared by the block) and selected, not branched on: the loads of
      // consecutive rows are then independent and in flight together; an unselected row adds an exact +0
#pragma unroll 8
      for (int r = 0; r < rows; ++r) {
        const float4 v = ld4(d + (long)r * C);
        const bool keep = (mw[r] & bit) != 0;
        a.x += keep ? v.x : 0.f; a.y += keep ? v.y : 0.f; a.z += keep ? v.z : 0.f; a.w += keep ? v.w : 0.f;
      }
      ct_acc[e] = a;
    }
  }
  float* out = part + ((long)s * B + b) * T * C;
  for (int e = tid; e < tc4; e += 256) st4q(out, e, ct_acc[e]);
}

int lotus_reduce_parts(const float* part, float* out, long n, long stride, int nz, int accumulate, hipStream_t st);  // gemm.hip

static int ct_check_shape(const char* who, int B, int n, int T, int C) {
  LOTUS_CHECK_ARG(C > 0 && C % 4 == 0, "%s: C = %d must be a positive multiple of 4", who, C);
  LOTUS_CHECK_ARG(T > 0 && T <= CT_TMAX, "%s: T = %d taps (1 <= T <= %d: two 64-bit presence words per row)", who, T, CT_TMAX);
  LOTUS_CHECK_ARG((long)T * C <= CT_MAX_TC, "%s: T x C = %d x %d floats do not fit LDS (T x C <= %d)", who, T, C, CT_MAX_TC);
  LOTUS_CHECK_ARG(B > 0 && B <= 65535, "%s: B = %d clouds (1 <= B <= 65535)", who, B);
  LOTUS_CHECK_ARG(n >= 0, "%s: n = %d rows must not be negative", who, n);
  return LOTUS_OK;
}

static int ct_lds(const char* who, const void* kernel, size_t lds) {
  // (from 48 KB on: the forward kernel adds 2 KB of static LDS to its dynamic part, and the default limit is 64 KB in all)
  if (lds > 49152 && hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    lotus_set_error("%s: launch failed: %zu bytes of LDS refused", who, lds);
    return LOTUS_E_LAUNCH;
  }
  return LOTUS_OK;
}

extern "C" {

size_t lotus_ctx_taps_workspace(int B, int T, int C) {
  return (size_t)CT_SPLITS * (B > 0 ? B : 1) * (T > 0 ? T : 1) * (C > 0 ? C : 4) * sizeof(float);
}

int lotus_ctx_taps_plan(int n, int B, int T, int C, int* out) {
  LOTUS_CHECK_ARG(out, "lotus_ctx_taps_plan: null pointer");
  const int rc = ct_check_shape("lotus_ctx_taps_plan", B, n, T, C);
  if (rc) return rc;
  out[0] = CT_ROWS; out[1] = cdiv(n, CT_ROWS); out[2] = CT_SPLITS; out[3] = CT_ROWS; out[4] = CT_BTILE; out[5] = CT_MAX_TC / T / 4 * 4;
  return LOTUS_OK;
}

int lotus_ctx_taps_fwd(const float* P, const int* nbr, const int* off, const float* add, float* y, int B, int n, int T, int C,
                       void* stream) {
  LOTUS_CHECK_ARG(P && nbr && off && y, "lotus_ctx_taps_fwd: null pointer");
  const int rc = ct_check_shape("lotus_ctx_taps_fwd", B, n, T, C);
  if (rc) return rc;
  LOTUS_CHECK_ARG((((uintptr_t)P) | ((uintptr_t)add) | ((uintptr_t)y)) % 16 == 0, "lotus_ctx_taps_fwd: P, add and y must be 16-byte aligned");
  if (n == 0) return LOTUS_OK;
  const size_t lds = (size_t)T * C * sizeof(float);
  const int lr = ct_lds("lotus_ctx_taps_fwd", (const void*)ctx_taps_fwd_kernel, lds);
  if (lr) return lr;
  LOTUS_LAUNCH(ctx_taps_fwd_kernel, dim3(cdiv(n, CT_ROWS), B), dim3(256), lds, (hipStream_t)stream, P, nbr, off, add, y, n, T, C);
  LOTUS_LAUNCH_CHECK("lotus_ctx_taps_fwd");
  return LOTUS_OK;
}

int lotus_ctx_taps_bwd(const float* dy, const int* nbr, const int* off, float* dP, int B, int n, int T, int C, void* workspace,
                       size_t workspace_bytes, void* stream) {
  LOTUS_CHECK_ARG(dy && nbr && off && dP, "lotus_ctx_taps_bwd: null pointer");
  const int rc = ct_check_shape("lotus_ctx_taps_bwd", B, n, T, C);
  if (rc) return rc;
  LOTUS_CHECK_ARG((((uintptr_t)dy) | ((uintptr_t)dP)) % 16 == 0, "lotus_ctx_taps_bwd: dy and dP must be 16-byte aligned");
  LOTUS_CHECK_ARG(workspace && ((uintptr_t)workspace) % 16 == 0 && workspace_bytes >= lotus_ctx_taps_workspace(B, T, C),
                  "lotus_ctx_taps_bwd: workspace too small or misaligned (lotus_ctx_taps_workspace(B, T, C) bytes)");
  if (n == 0) return LOTUS_OK;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)T * C * sizeof(float) + (size_t)CT_BTILE * 2 * sizeof(ct_u64);
  const int lr = ct_lds("lotus_ctx_taps_bwd", (const void*)ctx_taps_bwd_kernel, lds);
  if (lr) return lr;
  StopEventOnLast stop_ev;
  LOTUS_LAUNCH(ctx_taps_bwd_kernel, dim3(CT_SPLITS, B), dim3(256), lds, st, dy, nbr, off, (float*)workspace, B, n, T, C);
  LOTUS_LAUNCH_CHECK("lotus_ctx_taps_bwd");
  const long slab = (long)B * T * C;
  stop_ev.last();
  return lotus_reduce_parts((const float*)workspace, dP, slab, slab, CT_SPLITS, 0, st);
}

}  // extern "C"

}  // namespace LOTUS_NS
