// lotus-hip: the coordinate term of SerializedAttention (PointTransformerV3/model.py:396-398, 484-495: add_coords_in_attn 'qkv' adds
// coords_proj(point.coord) to the normed rows before the qkv product, 'qk' adds it to the q and the k columns of the product).  With
// P = coords_proj.weight [Cw][3] and c_i the three float coordinates of row i:
//   forward:          y[i][j] += sum_k c_i[k] P[j % Cw][k],   j < W,  W = Cw ('qkv': the normed rows) or 2 Cw ('qk': q | k of [q | k | v])
//   weight gradient:  dP[c][k] = sum_i sum_{h: c + h Cw < W} dy[i][c + h Cw] c_i[k]
// fp32 only (no bf16-storage twin).  Forward is one streaming pass: a block takes CA_ROWS rows, holds P (as three float4 planes, one
// per coordinate) and the rows' coordinates in LDS, and consecutive lanes take consecutive column quads of a row (16-byte loads and
// stores; columns >= W of a row are never touched).  The weight gradient has no atomics: a block takes one of S row ranges and QX
// column quads; its 256 threads are QX quad lanes x RL = 256 / QX row lanes, a thread sums its rows (stride RL) in fp32 over at most
// CA_RPT rows at a time and folds every such chunk into float64; the row lanes of a block (LDS) and the S ranges (merge kernel) are
// then summed in float64 in ascending order, so reruns are bit-identical.
#include "common.h"

namespace LOTUS_NS {

#define CA_ROWS 64       // rows per block, forward
#define CA_RPT 16        // rows a thread sums in fp32 before the sum goes into its float64 accumulator, weight gradient
#define CA_SPLITS 256    // most row ranges of the weight gradient (the workspace is S x Cw x 3 doubles)
#define CA_MAX_C 2048    // P in LDS, forward: 3 x Cw floats = 24 KB

__global__ __launch_bounds__(256) void coord_add_fwd_kernel(float* __restrict__ y, long ld, int W, int Cw,
                                                            const float* __restrict__ coord, long coord_ld,
                                                            const float* __restrict__ P, int n) {
  LOTUS_T_PRIO();
  extern __shared__ float4 ca_p[];  // [3][Cw / 4] float4: plane k holds P[.][k]; then [CA_ROWS][3] coordinates
  const int tid = threadIdx.x, cw4 = Cw / 4, w4 = W / 4;
  float* cs = reinterpret_cast<float*>(ca_p + 3 * cw4);
  const long r0 = (long)blockIdx.x * CA_ROWS;
  const int rows = (int)(n - r0 < CA_ROWS ? n - r0 : CA_ROWS);
  for (int i = tid; i < 3 * cw4; i += 256) {
    const int k = i / cw4, q = i - k * cw4;
    const float* p = P + (long)q * 12 + k;
    ca_p[i] = make_float4(p[0], p[3], p[6], p[9]);
  }
  for (int i = tid; i < rows * 3; i += 256) {
    const int r = i / 3, k = i - r * 3;
    cs[i] = coord[(r0 + r) * coord_ld + k];
  }
  __syncthreads();
  const int items = rows * w4;
  for (int e = tid; e < items; e += 256) {
    const int r = e / w4, q = e - r * w4, qc = q >= cw4 ? q - cw4 : q;
    float* yr = y + (r0 + r) * ld;
    const float c0 = cs[3 * r], c1 = cs[3 * r + 1], c2 = cs[3 * r + 2];
    const float4 p0 = ca_p[qc], p1 = ca_p[cw4 + qc], p2 = ca_p[2 * cw4 + qc];
    float4 a = ld4q(yr, q);
    // (the product first, then the sum with the row: the reference's order)
    a.x += fmaf(c2, p2.x, fmaf(c1, p1.x, c0 * p0.x));
    a.y += fmaf(c2, p2.y, fmaf(c1, p1.y, c0 * p0.y));
    a.z += fmaf(c2, p2.z, fmaf(c1, p1.z, c0 * p0.z));
    a.w += fmaf(c2, p2.w, fmaf(c1, p1.w, c0 * p0.w));
    st4q(yr, q, a);
  }
}

__device__ __forceinline__ void ca_fma4(float4& a, const float4 v, float c) {
  a.x = fmaf(v.x, c, a.x); a.y = fmaf(v.y, c, a.y); a.z = fmaf(v.z, c, a.z); a.w = fmaf(v.w, c, a.w);
}

// range s = blockIdx.x of S, quads [blockIdx.y QX, + QX) -> part[s][Cw][3] doubles
template <int QX>
__global__ __launch_bounds__(256) void coord_add_wgrad_kernel(const float* __restrict__ dy, long ld, int W, int Cw,
                                                              const float* __restrict__ coord, long coord_ld, int n, int S,
                                                              double* __restrict__ part) {
  LOTUS_T_PRIO();
  constexpr int RL = 256 / QX;
  __shared__ double red[256 * 12];  // [row lane][quad lane][k][4]
  const int tid = threadIdx.x, x = tid % QX, yl = tid / QX, s = blockIdx.x;
  const int cw4 = Cw / 4, q = blockIdx.y * QX + x, nh = W / Cw;
  const long r0 = (long)n * s / S, r1 = (long)n * (s + 1) / S;
  double acc[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) acc[j] = 0.0;
  if (q < cw4) {
    const float* d = dy + 4 * q;
    for (long rb = r0 + yl; rb < r1; rb += (long)RL * CA_RPT) {
      float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0;
#pragma unroll 4
      for (int t = 0; t < CA_RPT; ++t) {
        const long r = rb + (long)t * RL;
        if (r >= r1) break;
        const float* cr = coord + r * coord_ld;
        const float c0 = cr[0], c1 = cr[1], c2 = cr[2];
        for (int h = 0; h < nh; ++h) {
          const float4 v = ld4(d + r * ld + (long)h * Cw);
          ca_fma4(a0, v, c0); ca_fma4(a1, v, c1); ca_fma4(a2, v, c2);
        }
      }
      acc[0] += (double)a0.x; acc[1] += (double)a0.y; acc[2] += (double)a0.z; acc[3] += (double)a0.w;
      acc[4] += (double)a1.x; acc[5] += (double)a1.y; acc[6] += (double)a1.z; acc[7] += (double)a1.w;
      acc[8] += (double)a2.x; acc[9] += (double)a2.y; acc[10] += (double)a2.z; acc[11] += (double)a2.w;
    }
  }
#pragma unroll
  for (int j = 0; j < 12; ++j) red[tid * 12 + j] = acc[j];
  __syncthreads();
  for (int o = tid; o < QX * 12; o += 256) {
    double sum = 0.0;
    for (int r = 0; r < RL; ++r) sum += red[r * QX * 12 + o];
    const int xx = o / 12, j = o - xx * 12, k = j / 4, m = j - k * 4, qq = blockIdx.y * QX + xx;
    if (qq < cw4) part[((long)s * Cw + 4 * qq + m) * 3 + k] = sum;
  }
}

__global__ __launch_bounds__(256) void coord_add_merge_kernel(const double* __restrict__ part, float* __restrict__ dP, int S, int len) {
  LOTUS_T_PRIO();
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= len) return;
  double sum = 0.0;
  for (int s = 0; s < S; ++s) sum += part[(long)s * len + e];
  dP[e] = (float)sum;
}

// quad lanes of the weight-gradient block: the smallest power of two that holds the Cw / 4 quads of a row, 64 at most
static int ca_qx(int Cw) {
  int qx = 1;
  while (qx < 64 && qx < Cw / 4) qx *= 2;
  return qx;
}

static int ca_splits(int n, int Cw) {
  const long per = (long)(256 / ca_qx(Cw)) * CA_RPT;  // rows of a range whose threads sum one fp32 chunk each
  const long s = (n + per - 1) / per;
  return s < 1 ? 1 : s > CA_SPLITS ? CA_SPLITS : (int)s;
}

static int ca_check_shape(const char* who, int n, int W, int Cw) {
  LOTUS_CHECK_ARG(Cw > 0 && Cw % 4 == 0, "%s: Cw = %d must be a positive multiple of 4", who, Cw);
  LOTUS_CHECK_ARG(Cw <= CA_MAX_C, "%s: Cw = %d > %d (the projection is held in LDS)", who, Cw, CA_MAX_C);
  LOTUS_CHECK_ARG(W == Cw || W == 2 * Cw, "%s: W = %d must be Cw or 2 Cw (Cw = %d)", who, W, Cw);
  LOTUS_CHECK_ARG(n >= 0, "%s: n = %d rows must not be negative", who, n);
  return LOTUS_OK;
}

extern "C" {

size_t lotus_coord_add_workspace(int n, int W, int Cw) {
  (void)W;
  if (Cw <= 0 || Cw % 4) Cw = 4;
  return (size_t)ca_splits(n > 0 ? n : 0, Cw) * Cw * 3 * sizeof(double);
}

int lotus_coord_add_plan(int n, int W, int Cw, int* out) {
  LOTUS_CHECK_ARG(out, "lotus_coord_add_plan: null pointer");
  const int rc = ca_check_shape("lotus_coord_add_plan", n, W, Cw);
  if (rc) return rc;
  const int qx = ca_qx(Cw);
  out[0] = CA_ROWS; out[1] = cdiv(n, CA_ROWS); out[2] = ca_splits(n, Cw); out[3] = CA_RPT; out[4] = qx; out[5] = 256 / qx;
  return LOTUS_OK;
}

int lotus_coord_add_fwd(float* y, long ld, int W, int Cw, const float* coord, long coord_ld, const float* P, int n, void* stream) {
  LOTUS_CHECK_ARG(y && coord && P, "lotus_coord_add_fwd: null pointer");
  const int rc = ca_check_shape("lotus_coord_add_fwd", n, W, Cw);
  if (rc) return rc;
  LOTUS_CHECK_ARG(ld >= W && ld % 4 == 0, "lotus_coord_add_fwd: ld = %ld (ld >= W = %d, ld %% 4 == 0)", ld, W);
  LOTUS_CHECK_ARG(coord_ld >= 3, "lotus_coord_add_fwd: coord_ld = %ld < 3", coord_ld);
  LOTUS_CHECK_ARG(((uintptr_t)y) % 16 == 0 && ((uintptr_t)coord) % 4 == 0 && ((uintptr_t)P) % 4 == 0,
                  "lotus_coord_add_fwd: y must be 16-byte aligned (coord, P: 4)");
  if (n == 0) return LOTUS_OK;
  const size_t lds = (size_t)3 * Cw * sizeof(float) + (size_t)CA_ROWS * 3 * sizeof(float);
  LOTUS_LAUNCH(coord_add_fwd_kernel, dim3(cdiv(n, CA_ROWS)), dim3(256), lds, (hipStream_t)stream, y, ld, W, Cw, coord, coord_ld, P, n);
  LOTUS_LAUNCH_CHECK("lotus_coord_add_fwd");
  return LOTUS_OK;
}

int lotus_coord_add_wgrad(const float* dy, long ld, int W, int Cw, const float* coord, long coord_ld, int n, float* dP,
                          void* workspace, size_t workspace_bytes, void* stream) {
  LOTUS_CHECK_ARG(dy && coord && dP, "lotus_coord_add_wgrad: null pointer");
  const int rc = ca_check_shape("lotus_coord_add_wgrad", n, W, Cw);
  if (rc) return rc;
  LOTUS_CHECK_ARG(ld >= W && ld % 4 == 0, "lotus_coord_add_wgrad: ld = %ld (ld >= W = %d, ld %% 4 == 0)", ld, W);
  LOTUS_CHECK_ARG(coord_ld >= 3, "lotus_coord_add_wgrad: coord_ld = %ld < 3", coord_ld);
  LOTUS_CHECK_ARG(((uintptr_t)dy) % 16 == 0 && ((uintptr_t)coord) % 4 == 0 && ((uintptr_t)dP) % 4 == 0,
                  "lotus_coord_add_wgrad: dy must be 16-byte aligned (coord, dP: 4)");
  LOTUS_CHECK_ARG(workspace && ((uintptr_t)workspace) % 8 == 0 && workspace_bytes >= lotus_coord_add_workspace(n, W, Cw),
                  "lotus_coord_add_wgrad: workspace too small or misaligned (lotus_coord_add_workspace(n, W, Cw) bytes)");
  hipStream_t st = (hipStream_t)stream;
  const int S = ca_splits(n, Cw), qx = ca_qx(Cw), len = Cw * 3;
  const dim3 grid(S, cdiv(Cw / 4, qx));
  double* part = (double*)workspace;
  StopEventOnLast stop_ev;
#define CA_WGRAD(QX) LOTUS_LAUNCH(coord_add_wgrad_kernel<QX>, grid, dim3(256), 0, st, dy, ld, W, Cw, coord, coord_ld, n, S, part)
  switch (qx) {
    case 1: CA_WGRAD(1); break;
    case 2: CA_WGRAD(2); break;
    case 4: CA_WGRAD(4); break;
    case 8: CA_WGRAD(8); break;
    case 16: CA_WGRAD(16); break;
    case 32: CA_WGRAD(32); break;
    default: CA_WGRAD(64); break;
  }
#undef CA_WGRAD
  LOTUS_LAUNCH_CHECK("lotus_coord_add_wgrad");
  stop_ev.last();
  LOTUS_LAUNCH(coord_add_merge_kernel, dim3(cdiv(len, 256)), dim3(256), 0, st, (const double*)part, dP, S, len);
  LOTUS_LAUNCH_CHECK("lotus_coord_add_wgrad");
  return LOTUS_OK;
}

}  // extern "C"

}  // namespace LOTUS_NS
