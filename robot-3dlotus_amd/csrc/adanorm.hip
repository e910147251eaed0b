// lotus-hip: adaptive (context-modulated) PDNorm LayerNorm / BatchNorm(+GELU), forward and backward — the norms of
// SimplePolicyPTV3AdaNorm (PointTransformerV3/model.py:257-303 with adaptive = True, decouple = False).  For norm j of width C
// and the cloud b(i) of row i, with [shift | scale] = Linear_j(SiLU(c_b)) (shift first, model.py:302):
//   LN site:  y_i = (xhat_i gamma + beta) * (1 + scale_b(i)) + shift_b(i)              (+ residual, CPE)
//   BN site:  y_i = act((xhat_i gamma + beta) * (1 + scale_b(i)) + shift_b(i))         (xhat from the BatchNorm statistics)
// Every parameter gradient follows from two per-(cloud, column) sums P_b = sum_{i in b} dz xhat, Q_b = sum_{i in b} dz:
//   dgamma = sum_b (1 + s_b) P_b, dbeta = sum_b (1 + s_b) Q_b, dscale_b = gamma P_b + beta Q_b, dshift_b = Q_b,
// and the BatchNorm backward's column sums are sum dxhat = gamma dbeta, sum dxhat xhat = gamma dgamma.  The sums come from a
// grid over (cloud, row chunk) — a block never straddles two clouds — whose per-block partials a second small kernel adds in
// fixed order: no atomics, bit-reproducible.  fp32 activations only (no bf16-storage twin).
// SyncBatchNorm (data parallel): a BN site runs statistics -> message -> apply with one fp64 message double[2C + 1] per direction,
// SUM all-reduced by the caller: forward (sum x, sum x^2, rows) from lotus_batchnorm_stats_fused, finished by
// lotus_adabn_apply_sums; backward (sum dxhat, sum dxhat xhat, rows) = (gamma dbeta, gamma dgamma, M) from lotus_adabn_bwd_stats —
// a cloud lives on one rank, so dmod and the LOCAL dgamma / dbeta are final there — consumed by lotus_adabn_bwd_apply_sums.
#include "common.h"

namespace LOTUS_NS {

// cloud of row r: the last b with off[b] <= r (off[0] = 0, off[B] = M; empty clouds are skipped)
__device__ __forceinline__ int ada_cloud(const int* __restrict__ off, int B, int r) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= r) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ float ada_group_sum(float v, int lpr) {
  for (int o = lpr >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------ LayerNorm forward
// ln_fwd_kernel's layout: a row is owned by LPR lanes (16/32/64); lane holds float4 #(l + j * LPR), j < NV <= 4.
struct AdaLnP {
  const float* x;
  const float* res;
  const float* gamma;
  const float* beta;
  const float* mod;  // [B][ld]: shift in columns 0..C-1, scale in C..2C-1
  const int* off;
  float* y;
  float* mean;
  float* rstd;
  int M, C, LPR, NV, B, ld;
  float eps;
};

__global__ __launch_bounds__(256) void adaln_fwd_kernel(AdaLnP p) {
  LOTUS_T_PRIO();
  const int rpb = 256 / p.LPR;
  const int row = blockIdx.x * rpb + threadIdx.x / p.LPR;
  const int l = threadIdx.x % p.LPR;
  const bool valid = row < p.M;
  const int c4 = p.C / 4;
  float4 v[4];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int q = l + j * p.LPR;
    if (valid && j < p.NV && q < c4) {
      v[j] = ld4q(p.x + (long)row * p.C, q);
      s += v[j].x + v[j].y + v[j].z + v[j].w;
    }
  }
  const float mean = ada_group_sum(s, p.LPR) / p.C;
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = l + j * p.LPR;
    if (valid && j < p.NV && q < c4) {
      const float a = v[j].x - mean, b = v[j].y - mean, c = v[j].z - mean, d = v[j].w - mean;
      ss += a * a + b * b + c * c + d * d;
    }
  }
  const float rstd = rsqrtf(ada_group_sum(ss, p.LPR) / p.C + p.eps);
  if (!valid) return;
  if (l == 0) {
    if (p.mean) p.mean[row] = mean;
    if (p.rstd) p.rstd[row] = rstd;
  }
  const float* md = p.mod + (long)ada_cloud(p.off, p.B, row) * p.ld;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = l + j * p.LPR;
    if (j < p.NV && q < c4) {
      const float4 g = ld4q(p.gamma, q), b = ld4q(p.beta, q);
      const float4 sh = ld4q(md, q), sc = ld4q(md + p.C, q);
      float4 o;
      o.x = ((v[j].x - mean) * rstd * g.x + b.x) * (1.f + sc.x) + sh.x;
      o.y = ((v[j].y - mean) * rstd * g.y + b.y) * (1.f + sc.y) + sh.y;
      o.z = ((v[j].z - mean) * rstd * g.z + b.z) * (1.f + sc.z) + sh.z;
      o.w = ((v[j].w - mean) * rstd * g.w + b.w) * (1.f + sc.w) + sh.w;
      if (p.res) {
        const float4 r = ld4q(p.res + (long)row * p.C, q);
        o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
      }
      st4q(p.y + (long)row * p.C, q, o);
    }
  }
}

// ------------------------------------------------------------------------------ per-cloud partials
// Block (k, b) covers rows off[b] + n_b k / G ... off[b] + n_b (k + 1) / G of cloud b (possibly none: it then writes zeros)
// and leaves part[(b G + k)][2][C] = (P, Q) of those rows.
__device__ __forceinline__ void ada_chunk(const int* __restrict__ off, int G, int& r0, int& r1) {
  const int b = blockIdx.y, k = blockIdx.x;
  const long a = off[b], n = off[b + 1] - a;
  r0 = (int)(a + n * k / G);
  r1 = (int)(a + n * (k + 1) / G);
}

struct AdaLnBwdP {
  const float* dy;
  const float* x;
  const float* mean;
  const float* rstd;
  const float* gamma;
  const float* mod;
  const int* off;
  const float* add;
  float* dx;
  float* part;
  int M, C, LPR, NV, B, ld, G;
};

// dx = LN'(dy; effective gain gamma (1 + s_b)) (+ add), and the (P, Q) partials of the block's chunk
__global__ __launch_bounds__(256) void adaln_bwd_kernel(AdaLnBwdP p) {
  LOTUS_T_PRIO();
  extern __shared__ float red[];  // [rpb][2][C]
  const int rpb = 256 / p.LPR;
  const int rslot = threadIdx.x / p.LPR, l = threadIdx.x % p.LPR;
  const int c4 = p.C / 4;
  const float* sc = p.mod + (long)blockIdx.y * p.ld + p.C;
  int r0, r1;
  ada_chunk(p.off, p.G, r0, r1);
  float4 pp[4], pq[4], ge[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    pp[j] = pq[j] = ge[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int q = l + j * p.LPR;
    if (j < p.NV && q < c4) {
      const float4 g = ld4q(p.gamma, q), s = ld4q(sc, q);
      ge[j] = make_float4(g.x * (1.f + s.x), g.y * (1.f + s.y), g.z * (1.f + s.z), g.w * (1.f + s.w));
    }
  }
  for (int row0 = r0; row0 < r1; row0 += rpb) {
    const int row = row0 + rslot;
    const bool valid = row < r1;
    const float mean = valid ? p.mean[row] : 0.f, rstd = valid ? p.rstd[row] : 0.f;
    float4 xh[4], g[4], av[4];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = l + j * p.LPR;
      xh[j] = g[j] = av[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (valid && j < p.NV && q < c4) {
        const float4 xv = ld4q(p.x + (long)row * p.C, q);
        const float4 dv = ld4q(p.dy + (long)row * p.C, q);
        if (p.add) av[j] = ld4q(p.add + (long)row * p.C, q);
        xh[j] = make_float4((xv.x - mean) * rstd, (xv.y - mean) * rstd, (xv.z - mean) * rstd, (xv.w - mean) * rstd);
        pp[j].x += dv.x * xh[j].x; pp[j].y += dv.y * xh[j].y; pp[j].z += dv.z * xh[j].z; pp[j].w += dv.w * xh[j].w;
        pq[j].x += dv.x; pq[j].y += dv.y; pq[j].z += dv.z; pq[j].w += dv.w;
        g[j] = make_float4(dv.x * ge[j].x, dv.y * ge[j].y, dv.z * ge[j].z, dv.w * ge[j].w);
        s1 += g[j].x + g[j].y + g[j].z + g[j].w;
        s2 += g[j].x * xh[j].x + g[j].y * xh[j].y + g[j].z * xh[j].z + g[j].w * xh[j].w;
      }
    }
    s1 = ada_group_sum(s1, p.LPR) / p.C;
    s2 = ada_group_sum(s2, p.LPR) / p.C;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = l + j * p.LPR;
      if (valid && j < p.NV && q < c4) {
        float4 o;
        o.x = rstd * (g[j].x - s1 - xh[j].x * s2) + av[j].x;
        o.y = rstd * (g[j].y - s1 - xh[j].y * s2) + av[j].y;
        o.z = rstd * (g[j].z - s1 - xh[j].z * s2) + av[j].z;
        o.w = rstd * (g[j].w - s1 - xh[j].w * s2) + av[j].w;
        st4q(p.dx + (long)row * p.C, q, o);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = l + j * p.LPR;
    if (j < p.NV && q < c4) {
      st4q(red + (long)(rslot * 2 + 0) * p.C, q, pp[j]);
      st4q(red + (long)(rslot * 2 + 1) * p.C, q, pq[j]);
    }
  }
  __syncthreads();
  float* dst = p.part + ((long)blockIdx.y * p.G + blockIdx.x) * 2 * p.C;
  for (int c = threadIdx.x; c < 2 * p.C; c += 256) {
    const int which = c / p.C, col = c % p.C;
    float s = 0.f;
    for (int r = 0; r < rpb; ++r) s += red[(long)(r * 2 + which) * p.C + col];
    dst[c] = s;
  }
}

struct AdaBnP {
  const float* dy;  // backward only
  const float* x;
  const float* mean;
  const float* invstd;
  const float* gamma;
  const float* beta;
  const float* mod;
  const int* off;
  const float* dgamma;  // backward apply: the reduced parameter gradients (column sums of the BatchNorm backward)
  const float* dbeta;
  float* y;  // forward: y; backward apply: dx
  float* part;
  int M, C, B, ld, G, act, training;
  // the split (SyncBatchNorm) passes, adabn_cols_kernel: `sums` is the all-reduced fp64 message.  Forward: (sum x, sum x^2, rows)
  // -> mean / invstd (written to out_mean / out_invstd for backward) and the running averages; backward: (sum dxhat,
  // sum dxhat xhat, rows) of ALL ranks.
  const double* sums;
  float* out_mean;
  float* out_invstd;
  float* running_mean;
  float* running_var;
  float eps, momentum;
};

// BatchNorm backward partials: dz = dy act'((xhat gamma + beta)(1 + s) + shift), P += dz xhat, Q += dz over the chunk
__global__ __launch_bounds__(256) void adabn_part_kernel(AdaBnP p) {
  LOTUS_T_PRIO();
  extern __shared__ float red[];  // [rslots][2][C]
  const int c4 = p.C / 4;
  const int tpr = c4 < 256 ? c4 : 256;
  const int rslots = 256 / tpr;
  const int rslot = threadIdx.x / tpr, l = threadIdx.x % tpr;
  const float* md = p.mod + (long)blockIdx.y * p.ld;
  int r0, r1;
  ada_chunk(p.off, p.G, r0, r1);
  for (int q0 = 0; q0 < c4; q0 += tpr) {
    const int q = q0 + l;
    float4 sp = make_float4(0.f, 0.f, 0.f, 0.f), sq = sp;
    if (rslot < rslots && q < c4) {
      const float4 mu = ld4q(p.mean, q), is = ld4q(p.invstd, q), gm = ld4q(p.gamma, q), bt = ld4q(p.beta, q);
      const float4 sh = ld4q(md, q), sc = ld4q(md + p.C, q);
      const float m4[4] = {mu.x, mu.y, mu.z, mu.w}, i4[4] = {is.x, is.y, is.z, is.w};
      const float g4[4] = {gm.x, gm.y, gm.z, gm.w}, b4[4] = {bt.x, bt.y, bt.z, bt.w};
      const float h4[4] = {sh.x, sh.y, sh.z, sh.w}, s4[4] = {sc.x, sc.y, sc.z, sc.w};
      float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
      for (int row = r0 + rslot; row < r1; row += rslots) {
        const float4 xv = ld4q(p.x + (long)row * p.C, q), dv = ld4q(p.dy + (long)row * p.C, q);
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, ds[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xh = (xs[e] - m4[e]) * i4[e];
          const float z = (xh * g4[e] + b4[e]) * (1.f + s4[e]) + h4[e];
          const float dz = ds[e] * act_grad_f(z, p.act);
          a0[e] += dz * xh;
          a1[e] += dz;
        }
      }
      sp = make_float4(a0[0], a0[1], a0[2], a0[3]);
      sq = make_float4(a1[0], a1[1], a1[2], a1[3]);
    }
    __syncthreads();  // (red is reused per column slab)
    if (rslot < rslots && q < c4) {
      st4q(red + (long)(rslot * 2 + 0) * p.C, q, sp);
      st4q(red + (long)(rslot * 2 + 1) * p.C, q, sq);
    }
    __syncthreads();
    float* dst = p.part + ((long)blockIdx.y * p.G + blockIdx.x) * 2 * p.C;
    for (int t = threadIdx.x; t < 2 * 4 * tpr; t += 256) {
      const int which = t / (4 * tpr), col = q0 * 4 + t % (4 * tpr);
      if (col < p.C) {
        float s = 0.f;
        for (int r = 0; r < rslots; ++r) s += red[(long)(r * 2 + which) * p.C + col];
        dst[which * p.C + col] = s;
      }
    }
  }
}

// Fixed-order reduction of the (P, Q) partials: dmod[b] = (Q_b, gamma P_b + beta Q_b), dgamma = sum_b (1 + s_b) P_b,
// dbeta = sum_b (1 + s_b) Q_b.  Block = 64 columns x 4 cloud lanes (cloud lane t takes b = t, t + 4, ...), combined in LDS.
// SUMS (the SyncBatchNorm backward, lotus_adabn_bwd_stats): also the fp64 message sums[2C + 1] = (gamma dbeta, gamma dgamma, M) =
// (sum dxhat, sum dxhat xhat, rows) of the local rows, products and the sum over clouds formed in double from the fp32 P_b, Q_b.
template <bool SUMS>
__global__ __launch_bounds__(256) void ada_param_reduce_kernel(const float* __restrict__ part, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const float* __restrict__ mod, int ld,
                                                               float* __restrict__ dmod, int dld, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta, int B, int G, int C,
                                                               double* __restrict__ sums, int M) {
  __shared__ float red[2][4][64];
  __shared__ double dred[2][4][64];  // (SUMS only)
  const int cl = threadIdx.x & 63, t = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  float sg = 0.f, sb = 0.f;
  double dsg = 0.0, dsb = 0.0;
  if (c < C) {
    const float g = gamma[c], bt = beta[c];
    for (int b = t; b < B; b += 4) {
      const float* pb = part + (long)b * G * 2 * C;
      float P = 0.f, Q = 0.f;
      for (int k = 0; k < G; ++k) {
        P += pb[(long)k * 2 * C + c];
        Q += pb[(long)k * 2 * C + C + c];
      }
      const float s1 = 1.f + mod[(long)b * ld + C + c];
      sg += s1 * P;
      sb += s1 * Q;
      if (SUMS) {
        const double d1 = 1.0 + (double)mod[(long)b * ld + C + c];
        dsg += d1 * (double)P;
        dsb += d1 * (double)Q;
      }
      dmod[(long)b * dld + c] = Q;
      dmod[(long)b * dld + C + c] = g * P + bt * Q;
    }
  }
  red[0][t][cl] = sg;
  red[1][t][cl] = sb;
  if (SUMS) {
    dred[0][t][cl] = dsg;
    dred[1][t][cl] = dsb;
  }
  __syncthreads();
  if (t == 0 && c < C) {
    dgamma[c] = ((red[0][0][cl] + red[0][1][cl]) + red[0][2][cl]) + red[0][3][cl];
    dbeta[c] = ((red[1][0][cl] + red[1][1][cl]) + red[1][2][cl]) + red[1][3][cl];
    if (SUMS) {
      const double g = (double)gamma[c];
      sums[c] = g * (((dred[1][0][cl] + dred[1][1][cl]) + dred[1][2][cl]) + dred[1][3][cl]);
      sums[C + c] = g * (((dred[0][0][cl] + dred[0][1][cl]) + dred[0][2][cl]) + dred[0][3][cl]);
    }
  }
  if (SUMS && blockIdx.x == 0 && threadIdx.x == 0) sums[2 * C] = (double)M;
}

// BatchNorm apply: y = act((xhat gamma + beta)(1 + s_b) + shift_b); backward (p.dy): dx = invstd (dxhat - sum dxhat / M -
// xhat sum(dxhat xhat) / M) in training, invstd dxhat in eval, with dxhat = dy act'(.) (1 + s_b) gamma.
__global__ __launch_bounds__(256) void adabn_apply_kernel(AdaBnP p) {
  LOTUS_T_PRIO();
  const int c4 = p.C / 4;
  const long total4 = (long)p.M * c4;
  const float inv_m = p.M > 0 ? 1.f / (float)p.M : 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
    const int row = (int)(i / c4), q = (int)(i % c4);
    const float* md = p.mod + (long)ada_cloud(p.off, p.B, row) * p.ld;
    const float4 xv = ld4q(p.x, i), mu = ld4q(p.mean, q), is = ld4q(p.invstd, q), gm = ld4q(p.gamma, q), bt = ld4q(p.beta, q);
    const float4 sh = ld4q(md, q), sc = ld4q(md + p.C, q);
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, m4[4] = {mu.x, mu.y, mu.z, mu.w}, i4[4] = {is.x, is.y, is.z, is.w};
    const float g4[4] = {gm.x, gm.y, gm.z, gm.w}, b4[4] = {bt.x, bt.y, bt.z, bt.w};
    const float h4[4] = {sh.x, sh.y, sh.z, sh.w}, s4[4] = {sc.x, sc.y, sc.z, sc.w};
    float o[4];
    if (!p.dy) {
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = act_f(((xs[e] - m4[e]) * i4[e] * g4[e] + b4[e]) * (1.f + s4[e]) + h4[e], p.act);
    } else {
      const float4 dv = ld4q(p.dy, i), dg = ld4q(p.dgamma, q), db = ld4q(p.dbeta, q);
      const float ds[4] = {dv.x, dv.y, dv.z, dv.w}, dg4[4] = {dg.x, dg.y, dg.z, dg.w}, db4[4] = {db.x, db.y, db.z, db.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = (xs[e] - m4[e]) * i4[e];
        const float z = (xh * g4[e] + b4[e]) * (1.f + s4[e]) + h4[e];
        const float dxh = ds[e] * act_grad_f(z, p.act) * (1.f + s4[e]) * g4[e];
        o[e] = p.training ? i4[e] * (dxh - (g4[e] * db4[e]) * inv_m - xh * (g4[e] * dg4[e]) * inv_m) : i4[e] * dxh;
      }
    }
    st4q(p.y, i, make_float4(o[0], o[1], o[2], o[3]));
  }
}

// The apply passes of the split BatchNorm (statistics -> message -> apply), forward and backward, from the all-reduced fp64
// message p.sums.  The launch makes gridDim.x * 256 a multiple of C / 4 (ada_cols_grid), so a thread keeps ONE column quad for its
// whole grid-stride walk: the column constants — with their fp64 divisions — are formed once per thread, only the cloud's
// [shift | scale] is looked up per row.  Forward: the arithmetic of bn_finalize_kernel (norm.hip) with the GLOBAL row count; the
// threads of the first quad row also write mean / invstd for backward and update the running averages (M == 0: nothing else).
// Backward: dx = invstd (dxhat - S1 / M_all - xhat S2 / M_all), dxhat = dy act'(.) (1 + s_b) gamma.
__global__ __launch_bounds__(256) void adabn_cols_kernel(AdaBnP p) {
  LOTUS_T_PRIO();
  const int c4 = p.C / 4;
  const long total4 = (long)p.M * c4;
  const long i0 = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
  const bool first = !p.dy && i0 < c4;
  if (i0 >= total4 && !first) return;
  const int q = (int)(i0 % c4);
  float m4[4], i4[4], a4[4] = {0.f, 0.f, 0.f, 0.f}, b4m[4] = {0.f, 0.f, 0.f, 0.f};
  const double count = p.sums[2 * p.C];
  if (!p.dy) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = q * 4 + e;
      const double m = p.sums[c] / count;
      double var = p.sums[p.C + c] / count - m * m;
      if (var < 0) var = 0;
      m4[e] = (float)m;
      i4[e] = (float)(1.0 / sqrt(var + (double)p.eps));
      if (first) {
        p.out_mean[c] = m4[e];
        p.out_invstd[c] = i4[e];
        if (p.running_mean) {
          const double unbiased = count > 1 ? var * count / (count - 1) : var;
          p.running_mean[c] = (1.f - p.momentum) * p.running_mean[c] + p.momentum * (float)m;
          p.running_var[c] = (1.f - p.momentum) * p.running_var[c] + p.momentum * (float)unbiased;
        }
      }
    }
  } else {
    const float4 mu = ld4q(p.mean, q), is = ld4q(p.invstd, q);
    m4[0] = mu.x; m4[1] = mu.y; m4[2] = mu.z; m4[3] = mu.w;
    i4[0] = is.x; i4[1] = is.y; i4[2] = is.z; i4[3] = is.w;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a4[e] = (float)(p.sums[q * 4 + e] / count);
      b4m[e] = (float)(p.sums[p.C + q * 4 + e] / count);
    }
  }
  const float4 gm = ld4q(p.gamma, q), bt = ld4q(p.beta, q);
  const float g4[4] = {gm.x, gm.y, gm.z, gm.w}, b4[4] = {bt.x, bt.y, bt.z, bt.w};
  const int drow = (int)(step / c4);  // (the column quad is fixed: a grid step is a whole number of rows)
  int row = (int)(i0 / c4);
  for (long i = i0; i < total4; i += step, row += drow) {
    const float* md = p.mod + (long)ada_cloud(p.off, p.B, row) * p.ld;
    const float4 xv = ld4q(p.x, i), sh = ld4q(md, q), sc = ld4q(md + p.C, q);
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, h4[4] = {sh.x, sh.y, sh.z, sh.w}, s4[4] = {sc.x, sc.y, sc.z, sc.w};
    float o[4];
    if (!p.dy) {
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = act_f(((xs[e] - m4[e]) * i4[e] * g4[e] + b4[e]) * (1.f + s4[e]) + h4[e], p.act);
    } else {
      const float4 dv = ld4q(p.dy, i);
      const float ds[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = (xs[e] - m4[e]) * i4[e];
        const float z = (xh * g4[e] + b4[e]) * (1.f + s4[e]) + h4[e];
        const float dxh = ds[e] * act_grad_f(z, p.act) * (1.f + s4[e]) * g4[e];
        o[e] = i4[e] * (dxh - a4[e] - xh * b4m[e]);
      }
    }
    st4q(p.y, i, make_float4(o[0], o[1], o[2], o[3]));
  }
}

// y = SiLU(x), or with dy: y = dy SiLU'(x)
__global__ __launch_bounds__(256) void ada_silu_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ y,
                                                       long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = x[i];
    const float sg = 1.f / (1.f + __expf(-v));
    y[i] = dy ? dy[i] * sg * (1.f + v * (1.f - sg)) : v * sg;
  }
}

static int ada_geometry(int C, int* LPR, int* NV) {  // = ln_geometry of norm.hip
  if (C <= 0 || C % 4) return -1;
  const int c4 = C / 4;
  int lpr = 64;
  if (c4 <= 16) lpr = 16;
  else if (c4 <= 32) lpr = 32;
  const int nv = (c4 + lpr - 1) / lpr;
  if (nv > 4) return -1;
  *LPR = lpr;
  *NV = nv;
  return 0;
}

// row chunks per cloud: ~256 rows per block on average, at most 64 (the reduction reads B G partial rows per column)
static int ada_chunks(int M, int B) {
  int g = cdiv(M > 0 ? M : 1, (long)(B > 0 ? B : 1) * 256);
  return g < 1 ? 1 : (g > 64 ? 64 : g);
}

static int ada_grid(long total4, int* capped_out = nullptr) {
  long g = (total4 + 511) / 512;
  if (capped_out) *capped_out = g > 4096;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// adabn_cols_kernel: ada_grid rounded up to whole column periods (gridDim.x * 256 a multiple of C / 4, and >= C / 4 threads)
static int ada_cols_grid(long total4, int C) {
  const int c4 = C / 4;
  int a = 256, b = c4;
  while (b) { const int t = a % b; a = b; b = t; }  // a = gcd(256, c4)
  const int unit = c4 / a;
  return (ada_grid(total4) + unit - 1) / unit * unit;
}

}  // namespace LOTUS_NS

using namespace LOTUS_NS;

extern "C" {

size_t lotus_adanorm_workspace(int M, int B, int C) {
  if (C <= 0) return 0;
  return (size_t)(B > 0 ? B : 1) * ada_chunks(M, B) * 2 * C * sizeof(float);
}

// The launch plan of the kernels below for M rows in B clouds at width C, from the helpers the launches themselves use:
// out[6] = {row chunks per cloud G, grid of the elementwise apply kernels, grid of the column-period apply kernels (the split
// BatchNorm), 1 when the 4096-block cap was hit, lanes per row, quads per lane of the LayerNorm site (0, 0: the LayerNorm
// entry points refuse the width, the BatchNorm ones take it)}.
int lotus_adanorm_plan(int M, int B, int C, int* out) {
  LOTUS_CHECK_ARG(out && M >= 0 && B > 0 && C > 0 && C % 4 == 0 && C <= 4096, "lotus_adanorm_plan: bad arguments (B=%d, C=%d)", B, C);
  const long total4 = (long)M * C / 4;
  out[0] = ada_chunks(M, B);
  out[1] = ada_grid(total4, out + 3);
  out[2] = ada_cols_grid(total4, C);
  if (ada_geometry(C, out + 4, out + 5)) out[4] = out[5] = 0;
  return LOTUS_OK;
}

int lotus_adaln_fwd(const float* x, const float* res, const float* gamma, const float* beta, const float* mod, int mod_ld,
                    const int* off, int B, float* y, float* mean, float* rstd, int M, int C, float eps, void* stream) {
  AdaLnP p;
  p.x = x; p.res = res; p.gamma = gamma; p.beta = beta; p.mod = mod; p.off = off; p.y = y; p.mean = mean; p.rstd = rstd;
  p.M = M; p.C = C; p.B = B; p.ld = mod_ld; p.eps = eps;
  LOTUS_CHECK_ARG(x && gamma && beta && mod && off && y && M >= 0 && B > 0 && mod_ld >= 2 * C, "lotus_adaln_fwd: bad arguments");
  LOTUS_CHECK_ARG(ada_geometry(C, &p.LPR, &p.NV) == 0, "lotus_adaln_fwd: unsupported C=%d", C);
  if (M == 0) return LOTUS_OK;
  LOTUS_LAUNCH(adaln_fwd_kernel, dim3(cdiv(M, 256 / p.LPR)), dim3(256), 0, (hipStream_t)stream, p);
  LOTUS_LAUNCH_CHECK("lotus_adaln_fwd");
  return LOTUS_OK;
}

int lotus_adaln_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                    const float* mod, int mod_ld, const int* off, int B, const float* add, float* dx, float* dgamma, float* dbeta,
                    float* dmod, int dmod_ld, int M, int C, void* workspace, size_t workspace_bytes, void* stream) {
  AdaLnBwdP p;
  p.dy = dy; p.x = x; p.mean = mean; p.rstd = rstd; p.gamma = gamma; p.mod = mod; p.off = off; p.add = add; p.dx = dx;
  p.part = (float*)workspace; p.M = M; p.C = C; p.B = B; p.ld = mod_ld; p.G = ada_chunks(M, B);
  LOTUS_CHECK_ARG(dy && x && mean && rstd && gamma && beta && mod && off && dx && dgamma && dbeta && dmod && M >= 0 && B > 0 &&
                  mod_ld >= 2 * C && dmod_ld >= 2 * C, "lotus_adaln_bwd: bad arguments");
  LOTUS_CHECK_ARG(ada_geometry(C, &p.LPR, &p.NV) == 0, "lotus_adaln_bwd: unsupported C=%d", C);
  LOTUS_CHECK_ARG(workspace && workspace_bytes >= lotus_adanorm_workspace(M, B, C), "lotus_adaln_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  LOTUS_LAUNCH(adaln_bwd_kernel, dim3(p.G, B), dim3(256), (size_t)(256 / p.LPR) * 2 * C * sizeof(float), st, p);
  LOTUS_LAUNCH(ada_param_reduce_kernel<false>, dim3(cdiv(C, 64)), dim3(256), 0, st, p.part, gamma, beta, mod, mod_ld, dmod, dmod_ld,
               dgamma, dbeta, B, p.G, C, (double*)nullptr, M);
  LOTUS_LAUNCH_CHECK("lotus_adaln_bwd");
  return LOTUS_OK;
}

int lotus_adabn_apply(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta, const float* mod,
                      int mod_ld, const int* off, int B, float* y, int M, int C, int act, void* stream) {
  LOTUS_CHECK_ARG(x && mean && invstd && gamma && beta && mod && off && y && M >= 0 && B > 0 && C > 0 && C % 4 == 0 && mod_ld >= 2 * C,
                  "lotus_adabn_apply: bad arguments");
  if (M == 0) return LOTUS_OK;
  AdaBnP p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.mean = mean; p.invstd = invstd; p.gamma = gamma; p.beta = beta; p.mod = mod; p.off = off; p.y = y;
  p.M = M; p.C = C; p.B = B; p.ld = mod_ld; p.act = act;
  LOTUS_LAUNCH(adabn_apply_kernel, dim3(ada_grid((long)M * C / 4)), dim3(256), 0, (hipStream_t)stream, p);
  LOTUS_LAUNCH_CHECK("lotus_adabn_apply");
  return LOTUS_OK;
}

int lotus_adabn_bwd(const float* dy, const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                    const float* mod, int mod_ld, const int* off, int B, float* dx, float* dgamma, float* dbeta, float* dmod,
                    int dmod_ld, int M, int C, int act, int training, void* workspace, size_t workspace_bytes, void* stream) {
  LOTUS_CHECK_ARG(dy && x && mean && invstd && gamma && beta && mod && off && dx && dgamma && dbeta && dmod && M >= 0 && B > 0 &&
                  C > 0 && C % 4 == 0 && C <= 4096 && mod_ld >= 2 * C && dmod_ld >= 2 * C, "lotus_adabn_bwd: bad arguments");
  LOTUS_CHECK_ARG(workspace && workspace_bytes >= lotus_adanorm_workspace(M, B, C), "lotus_adabn_bwd: workspace too small");
  AdaBnP p;
  memset(&p, 0, sizeof(p));
  p.dy = dy; p.x = x; p.mean = mean; p.invstd = invstd; p.gamma = gamma; p.beta = beta; p.mod = mod; p.off = off;
  p.dgamma = dgamma; p.dbeta = dbeta; p.y = dx; p.part = (float*)workspace;
  p.M = M; p.C = C; p.B = B; p.ld = mod_ld; p.G = ada_chunks(M, B); p.act = act; p.training = training;
  hipStream_t st = (hipStream_t)stream;
  const int c4 = C / 4, tpr = c4 < 256 ? c4 : 256;
  LOTUS_LAUNCH(adabn_part_kernel, dim3(p.G, B), dim3(256), (size_t)(256 / tpr) * 2 * C * sizeof(float), st, p);
  LOTUS_LAUNCH(ada_param_reduce_kernel<false>, dim3(cdiv(C, 64)), dim3(256), 0, st, p.part, gamma, beta, mod, mod_ld, dmod, dmod_ld,
               dgamma, dbeta, B, p.G, C, (double*)nullptr, M);
  if (M > 0) LOTUS_LAUNCH(adabn_apply_kernel, dim3(ada_grid((long)M * C / 4)), dim3(256), 0, st, p);
  LOTUS_LAUNCH_CHECK("lotus_adabn_bwd");
  return LOTUS_OK;
}

// Forward from the (all-reduced) statistics sums = (sum x, sum x^2, rows): mean / invstd (saved for backward), the running
// averages and the modulated apply pass in one launch.  M == 0 (an empty shard): the statistics alone.
int lotus_adabn_apply_sums(const float* x, const double* sums, const float* gamma, const float* beta, const float* mod, int mod_ld,
                           const int* off, int B, float* y, float* mean, float* invstd, float* running_mean, float* running_var,
                           int M, int C, int act, float eps, float momentum, void* stream) {
  LOTUS_CHECK_ARG(sums && gamma && beta && mean && invstd && (!running_mean == !running_var) && M >= 0 && C > 0 && C % 4 == 0 &&
                  (M == 0 || (x && y && mod && off && B > 0 && mod_ld >= 2 * C)), "lotus_adabn_apply_sums: bad arguments");
  AdaBnP p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.gamma = gamma; p.beta = beta; p.mod = mod; p.off = off; p.y = y;
  p.M = M; p.C = C; p.B = B; p.ld = mod_ld; p.act = act;
  p.sums = sums; p.out_mean = mean; p.out_invstd = invstd; p.running_mean = running_mean; p.running_var = running_var;
  p.eps = eps; p.momentum = momentum;
  LOTUS_LAUNCH(adabn_cols_kernel, dim3(ada_cols_grid((long)M * C / 4, C)), dim3(256), 0, (hipStream_t)stream, p);
  LOTUS_LAUNCH_CHECK("lotus_adabn_apply_sums");
  return LOTUS_OK;
}

// Backward, first half: the (cloud, chunk) partials and their fixed-order reduction as in lotus_adabn_bwd — dgamma, dbeta (LOCAL
// sums) and dmod are final — plus the fp64 message sums[2C + 1] = (gamma dbeta, gamma dgamma, M) of the local rows.
int lotus_adabn_bwd_stats(const float* dy, const float* x, const float* mean, const float* invstd, const float* gamma,
                          const float* beta, const float* mod, int mod_ld, const int* off, int B, float* dgamma, float* dbeta,
                          float* dmod, int dmod_ld, double* sums, int M, int C, int act, void* workspace, size_t workspace_bytes,
                          void* stream) {
  LOTUS_CHECK_ARG(mean && invstd && gamma && beta && mod && off && dgamma && dbeta && dmod && sums && M >= 0 && B > 0 && C > 0 &&
                  C % 4 == 0 && C <= 4096 && mod_ld >= 2 * C && dmod_ld >= 2 * C && (M == 0 || (dy && x)),
                  "lotus_adabn_bwd_stats: bad arguments");
  LOTUS_CHECK_ARG(workspace && workspace_bytes >= lotus_adanorm_workspace(M, B, C), "lotus_adabn_bwd_stats: workspace too small");
  AdaBnP p;
  memset(&p, 0, sizeof(p));
  p.dy = dy; p.x = x; p.mean = mean; p.invstd = invstd; p.gamma = gamma; p.beta = beta; p.mod = mod; p.off = off;
  p.part = (float*)workspace; p.M = M; p.C = C; p.B = B; p.ld = mod_ld; p.G = ada_chunks(M, B); p.act = act; p.training = 1;
  hipStream_t st = (hipStream_t)stream;
  const int c4 = C / 4, tpr = c4 < 256 ? c4 : 256;
  LOTUS_LAUNCH(adabn_part_kernel, dim3(p.G, B), dim3(256), (size_t)(256 / tpr) * 2 * C * sizeof(float), st, p);
  LOTUS_LAUNCH(ada_param_reduce_kernel<true>, dim3(cdiv(C, 64)), dim3(256), 0, st, p.part, gamma, beta, mod, mod_ld, dmod, dmod_ld,
               dgamma, dbeta, B, p.G, C, sums, M);
  LOTUS_LAUNCH_CHECK("lotus_adabn_bwd_stats");
  return LOTUS_OK;
}

// Backward, second half: dx from the all-reduced message (sum dxhat, sum dxhat xhat, rows of all ranks).
int lotus_adabn_bwd_apply_sums(const float* dy, const float* x, const float* mean, const float* invstd, const float* gamma,
                               const float* beta, const float* mod, int mod_ld, const int* off, int B, const double* sums, float* dx,
                               int M, int C, int act, void* stream) {
  LOTUS_CHECK_ARG(mean && invstd && gamma && beta && mod && off && sums && M >= 0 && B > 0 && C > 0 && C % 4 == 0 && mod_ld >= 2 * C &&
                  (M == 0 || (dy && x && dx)), "lotus_adabn_bwd_apply_sums: bad arguments");
  if (M == 0) return LOTUS_OK;
  AdaBnP p;
  memset(&p, 0, sizeof(p));
  p.dy = dy; p.x = x; p.mean = mean; p.invstd = invstd; p.gamma = gamma; p.beta = beta; p.mod = mod; p.off = off; p.y = dx;
  p.M = M; p.C = C; p.B = B; p.ld = mod_ld; p.act = act; p.training = 1; p.sums = sums;
  LOTUS_LAUNCH(adabn_cols_kernel, dim3(ada_cols_grid((long)M * C / 4, C)), dim3(256), 0, (hipStream_t)stream, p);
  LOTUS_LAUNCH_CHECK("lotus_adabn_bwd_apply_sums");
  return LOTUS_OK;
}

int lotus_ada_silu(const float* x, const float* dy, float* y, int n, void* stream) {
  LOTUS_CHECK_ARG(x && y && n >= 0, "lotus_ada_silu: bad arguments");
  if (n == 0) return LOTUS_OK;
  LOTUS_LAUNCH(ada_silu_kernel, dim3(cdiv(n, 256) < 1024 ? cdiv(n, 256) : 1024), dim3(256), 0, (hipStream_t)stream, x, dy, y, (long)n);
  LOTUS_LAUNCH_CHECK("lotus_ada_silu");
  return LOTUS_OK;
}

}  // extern "C"
