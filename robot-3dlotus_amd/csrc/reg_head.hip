// lotus-hip: the regression action head — pos_pred_type 'heatmap_mlp' and rot_pred_type 'euler' / 'quat' of
// genrobo3d/models/simple_policy_ptv3.py:46-53,83-103,142-152 with their losses (:322-368).  fp32 activations only (no
// bf16-storage twin).
//   position:  e = h W3^T + b3 [N][4];  per cloud b over its rows i:  p_i = softmax_i(e_i0 / temp),  q_i = coord_i + e_i[1:4],
//              xt_b = sum_i p_i q_i.   Backward with g_b = dL / dxt_b:  de_i[1:4] = p_i g_b,  de_i0 = p_i ((q_i - xt_b) . g_b) / temp.
//   losses:    pos = mean (xt - gt[:, :3])^2 (or the heat-map cross entropy of lotus_pos_ce_fwd), rot = closest-of-two MSE
//              ('euler': target and target -+ 2; 'quat': target and -target on the normalised prediction) or the euler_disc
//              cross entropy, open = BCE with logits, total = pos_w pos + rot_w rot + open.
// The 4-column product is formed in the pass that reads the row (float4 loads, 16 lanes per row, W3 in LDS): the pass is bound
// by reading h.  The softmax runs on a grid over (cloud, row chunk) — a block never straddles two clouds — whose (max, sum,
// weighted sums) partials a second small kernel merges in fixed order: no atomics, bit-reproducible, no host synchronisation.
// The sums are carried in double (as the heat-map cross entropy carries its log-sum-exp): every p_i of a
// cloud shares the error of its log-sum-exp.
#include "common.h"

namespace LOTUS_NS {

#define SP_SPLITS 32  // row chunks per cloud (<= 64: one wave merges them)
#define SP_PART 5     // doubles per chunk partial: max z, sum exp(z - max), sum exp(z - max) q[0..2]
#define SP_LPR 16     // lanes per row in the product pass

__device__ __forceinline__ double reg_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// chunk s of cloud b: e rows of the chunk, then the chunk's softmax partial (z = e0 / temp)
__global__ __launch_bounds__(256) void softpos_part_kernel(const float* __restrict__ h, const float* __restrict__ w3,
                                                           const float* __restrict__ b3, const float* __restrict__ pc, long ld,
                                                           const int* __restrict__ off, int C, double inv_temp,
                                                           float* __restrict__ e, double* __restrict__ part) {
  LOTUS_T_PRIO();
  extern __shared__ float4 sp_w[];  // W3 [4][C / 4] float4
  __shared__ float red[4];
  __shared__ double redd[4];
  const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n0 = off[b], nn = off[b + 1] - n0;
  const int p0 = n0 + (int)((long)nn * s / SP_SPLITS), p1 = n0 + (int)((long)nn * (s + 1) / SP_SPLITS);
  const int c4 = C / 4;
  if (p0 < p1) {
    for (int i = tid; i < 4 * c4; i += 256) sp_w[i] = ld4q(w3, i);
  }
  __syncthreads();
  const int l = tid % SP_LPR, g = tid / SP_LPR;
  const float4 bias = ld4(b3);
  float m = -INFINITY;
  for (int r0 = p0; r0 < p1; r0 += 256 / SP_LPR) {  // (uniform trip count: the shuffles below see every lane)
    const int row = r0 + g;
    const bool valid = row < p1;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (valid) {
      const float* hr = h + (long)row * C;
      for (int q = l; q < c4; q += SP_LPR) {
        const float4 x = ld4q(hr, q);
        const float4 u0 = sp_w[q], u1 = sp_w[c4 + q], u2 = sp_w[2 * c4 + q], u3 = sp_w[3 * c4 + q];
        a0 = fmaf(x.x, u0.x, fmaf(x.y, u0.y, fmaf(x.z, u0.z, fmaf(x.w, u0.w, a0))));
        a1 = fmaf(x.x, u1.x, fmaf(x.y, u1.y, fmaf(x.z, u1.z, fmaf(x.w, u1.w, a1))));
        a2 = fmaf(x.x, u2.x, fmaf(x.y, u2.y, fmaf(x.z, u2.z, fmaf(x.w, u2.w, a2))));
        a3 = fmaf(x.x, u3.x, fmaf(x.y, u3.y, fmaf(x.z, u3.z, fmaf(x.w, u3.w, a3))));
      }
    }
#pragma unroll
    for (int o = SP_LPR >> 1; o > 0; o >>= 1) {
      a0 += __shfl_xor(a0, o, 64); a1 += __shfl_xor(a1, o, 64); a2 += __shfl_xor(a2, o, 64); a3 += __shfl_xor(a3, o, 64);
    }
    if (valid && l == 0) {
      a0 += bias.x;
      st4(e + (long)row * 4, make_float4(a0, a1 + bias.y, a2 + bias.z, a3 + bias.w));
      m = fmaxf(m, a0);
    }
  }
  m = wave_max(m);
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();  // (also orders the e rows written above before the reads below: same block)
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const double zm = (double)m * inv_temp;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int row = p0 + tid; row < p1; row += 256) {
    const float4 er = ld4(e + (long)row * 4);
    const float* cr = pc + (long)row * ld;
    const double w = exp((double)er.x * inv_temp - zm);
    v[0] += w;
    v[1] += w * ((double)cr[0] + (double)er.y);
    v[2] += w * ((double)cr[1] + (double)er.z);
    v[3] += w * ((double)cr[2] + (double)er.w);
  }
  double tot[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double w = reg_wave_sum_d(v[k]);
    if ((tid & 63) == 0) redd[tid >> 6] = w;
    __syncthreads();
    tot[k] = ((redd[0] + redd[1]) + redd[2]) + redd[3];
    __syncthreads();
  }
  if (tid == 0) {
    double* o = part + ((long)b * SP_SPLITS + s) * SP_PART;
    o[0] = p0 < p1 ? zm : -INFINITY;
    o[1] = tot[0]; o[2] = tot[1]; o[3] = tot[2]; o[4] = tot[3];
  }
}

// fixed-order merge of a cloud's chunks: xt[b] = sum p q, stats[b] = (max z, log-sum-exp of z)
__global__ __launch_bounds__(64) void softpos_merge_kernel(const double* __restrict__ part, float* __restrict__ xt,
                                                           double* __restrict__ stats) {
  LOTUS_T_PRIO();
  const int b = blockIdx.x, s = threadIdx.x;
  double m = -INFINITY, v[4] = {0.0, 0.0, 0.0, 0.0};
  if (s < SP_SPLITS) {
    const double* o = part + ((long)b * SP_SPLITS + s) * SP_PART;
    m = o[0]; v[0] = o[1]; v[1] = o[2]; v[2] = o[3]; v[3] = o[4];
  }
  double M = m;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) M = fmax(M, __shfl_xor(M, o, 64));
  const double sc = m > -INFINITY ? exp(m - M) : 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = reg_wave_sum_d(m > -INFINITY ? v[k] * sc : 0.0);
  if (s == 0) {
    xt[b * 3 + 0] = (float)(v[1] / v[0]);
    xt[b * 3 + 1] = (float)(v[2] / v[0]);
    xt[b * 3 + 2] = (float)(v[3] / v[0]);
    stats[b * 2 + 0] = M;
    stats[b * 2 + 1] = M + log(v[0]);
  }
}

// de [N][4] in one pass: p = exp(z - lse); de[1:4] = p g_b, de[0] = p ((q - xt_b) . g_b) / temp
__global__ __launch_bounds__(256) void softpos_bwd_kernel(const float* __restrict__ g, const float* __restrict__ e,
                                                          const float* __restrict__ pc, long ld, const int* __restrict__ batch,
                                                          const double* __restrict__ stats, const float* __restrict__ xt, int n,
                                                          double inv_temp, float* __restrict__ de) {
  LOTUS_T_PRIO();
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const int b = batch[row];
  const float4 er = ld4(e + (long)row * 4);
  const float* cr = pc + (long)row * ld;
  const double p = exp((double)er.x * inv_temp - stats[b * 2 + 1]);
  const double g0 = g[b * 3], g1 = g[b * 3 + 1], g2 = g[b * 3 + 2];
  const double d0 = ((double)cr[0] + (double)er.y) - (double)xt[b * 3];
  const double d1 = ((double)cr[1] + (double)er.z) - (double)xt[b * 3 + 1];
  const double d2 = ((double)cr[2] + (double)er.w) - (double)xt[b * 3 + 2];
  st4(de + (long)row * 4, make_float4((float)(p * (d0 * g0 + d1 * g1 + d2 * g2) * inv_temp), (float)(p * g0), (float)(p * g1),
                                      (float)(p * g2)));
}

// ---------------------------------------------------------------------------------------------------------------
// The [B]-sized losses in one block (simple_policy_ptv3.py:322-368).  ae [B][W]: rotation in the leading columns, openness
// logit in the LAST column; gt [B][ga]: position 0..2, rotation 3..ga-2, openness ga-1.  rot_kind 0 = euler_disc (W = nrot*3 + 1,
// logits (bin, axis) at bin*3 + axis), 1 = euler (columns 0..2), 2 = quat (columns 0..3, normalised into xr [B][4]).
// Position: xt [B][3] (heatmap_mlp: MSE) or ce with stride ce_ld (heatmap_disc: cross entropy per (cloud, axis)).
// losses[4] = pos, rot, open, total.  dae [B][W] and dpos [B][3] keep the partial derivatives of the loss each column belongs
// to (disjoint columns; columns of neither loss get an exact 0), unscaled by the upstream gradient.  gt == null: only xr.
struct RegLossP {
  const float* ae; const float* gt; const float* xt; const float* ce;
  float* losses; float* dae; float* dpos; float* xr;
  int B, W, ga, rot_kind, nrot, ce_ld;
  float pos_w, rot_w;
};

__global__ __launch_bounds__(256) void reg_loss_kernel(RegLossP p) {
  LOTUS_T_PRIO();
  __shared__ double red[3][4];
  const int tid = threadIdx.x, B = p.B, W = p.W, ga = p.ga;
  double pos = 0.0, rot = 0.0, opn = 0.0;
  if (p.rot_kind == 2) {
    for (int b = tid; b < B; b += 256) {
      const float* row = p.ae + (long)b * W;
      const double a[4] = {row[0], row[1], row[2], row[3]};
      const double nrm = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3]);  // (no epsilon, as the reference)
      double x[4];
      for (int k = 0; k < 4; ++k) {
        x[k] = a[k] / nrm;
        p.xr[b * 4 + k] = (float)x[k];
      }
      if (!p.gt) continue;
      const float* t = p.gt + (long)b * ga + 3;
      double la = 0.0, lb = 0.0;
      for (int k = 0; k < 4; ++k) {
        la += (x[k] - (double)t[k]) * (x[k] - (double)t[k]);
        lb += (x[k] + (double)t[k]) * (x[k] + (double)t[k]);
      }
      la *= 0.25; lb *= 0.25;
      const double sg = la < lb ? 1.0 : -1.0;
      rot += la < lb ? la : lb;
      double d[4], xd = 0.0;
      for (int k = 0; k < 4; ++k) {
        d[k] = 2.0 * (x[k] - sg * (double)t[k]) / (4.0 * B);
        xd += x[k] * d[k];
      }
      for (int k = 0; k < 4; ++k) p.dae[(long)b * W + k] = (float)((d[k] - x[k] * xd) / nrm);
      for (int k = 4; k < W - 1; ++k) p.dae[(long)b * W + k] = 0.f;
    }
  }
  if (!p.gt) return;
  if (p.rot_kind == 1) {
    for (int b = tid; b < B; b += 256) {
      for (int k = 0; k < 3; ++k) {
        const double x = p.ae[(long)b * W + k], t = p.gt[(long)b * ga + 3 + k];
        const double alt = t < 0.0 ? t + 2.0 : t > 0.0 ? t - 2.0 : t;
        const double la = (x - t) * (x - t), lb = (x - alt) * (x - alt);
        const double tt = la < lb ? t : alt;
        rot += la < lb ? la : lb;
        p.dae[(long)b * W + k] = (float)(2.0 * (x - tt) / (3.0 * B));
      }
      for (int k = 3; k < W - 1; ++k) p.dae[(long)b * W + k] = 0.f;
    }
  } else if (p.rot_kind == 0) {
    const int nrot = p.nrot;
    for (int i = tid; i < B * 3; i += 256) {
      const int b = i / 3, a = i % 3;
      const float* row = p.ae + (long)b * W;
      float mx = -INFINITY;
      for (int k = 0; k < nrot; ++k) mx = fmaxf(mx, row[k * 3 + a]);
      double se = 0.0;
      for (int k = 0; k < nrot; ++k) se += exp((double)row[k * 3 + a] - (double)mx);
      const double lse = (double)mx + log(se);
      const int tk = min(max((int)p.gt[(long)b * ga + 3 + a], 0), nrot - 1);
      rot += lse - (double)row[tk * 3 + a];
      for (int k = 0; k < nrot; ++k)
        p.dae[(long)b * W + k * 3 + a] = (float)((exp((double)row[k * 3 + a] - lse) - (k == tk ? 1.0 : 0.0)) / (3.0 * B));
    }
  }
  for (int i = tid; i < B * 3; i += 256) {
    if (p.xt) {
      const double d = (double)p.xt[i] - (double)p.gt[(long)(i / 3) * ga + i % 3];
      pos += d * d;
      p.dpos[i] = (float)(2.0 * d / (3.0 * B));
    } else {
      pos += (double)p.ce[(long)i * p.ce_ld];
      p.dpos[i] = (float)(1.0 / (3.0 * B));
    }
  }
  for (int b = tid; b < B; b += 256) {
    const double x = p.ae[(long)b * W + W - 1], t = p.gt[(long)b * ga + ga - 1];
    opn += fmax(x, 0.0) - x * t + log1p(exp(-fabs(x)));
    p.dae[(long)b * W + W - 1] = (float)((1.0 / (1.0 + exp(-x)) - t) / B);
  }
  const double v3[3] = {pos, rot, opn};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double w = reg_wave_sum_d(v3[k]);
    if ((tid & 63) == 0) red[k][tid >> 6] = w;
  }
  __syncthreads();
  if (tid == 0) {
    double t3[3];
    for (int k = 0; k < 3; ++k) t3[k] = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
    const double lp = t3[0] / (3.0 * B), lr = t3[1] / (p.rot_kind == 2 ? (double)B : 3.0 * B), lo = t3[2] / B;
    p.losses[0] = (float)lp; p.losses[1] = (float)lr; p.losses[2] = (float)lo;
    p.losses[3] = (float)((double)p.pos_w * lp + (double)p.rot_w * lr + lo);
  }
}

// upstream gradient gl[4] (device) of the four losses -> d ae [B][W], d pos [B][3]
__global__ void reg_loss_bwd_kernel(const float* __restrict__ dae, const float* __restrict__ dpos, const float* __restrict__ gl,
                                    float pos_w, float rot_w, int W, long nae, long npos, float* __restrict__ dae_out,
                                    float* __restrict__ dpos_out) {
  LOTUS_T_PRIO();
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nae) dae_out[i] = dae[i] * ((int)(i % W) == W - 1 ? gl[2] + gl[3] : gl[1] + rot_w * gl[3]);
  if (i < npos) dpos_out[i] = dpos[i] * (gl[0] + pos_w * gl[3]);
}

extern "C" {

size_t lotus_softpos_workspace(int B) { return (size_t)(B > 0 ? B : 1) * SP_SPLITS * SP_PART * sizeof(double); }

int lotus_softpos_fwd(const float* h, const float* w3, const float* b3, const float* pc, long ld, const int* off, int B, int n,
                      int C, double temp, float* e, float* xt, double* stats, void* workspace, size_t workspace_bytes,
                      void* stream) {
  LOTUS_CHECK_ARG(h && w3 && b3 && pc && off && e && xt && stats && B > 0 && n > 0 && C >= 4 && C % 4 == 0 && ld >= 3 && temp > 0.0,
                  "lotus_softpos_fwd: bad arguments (C %% 4 == 0, ld >= 3, temp > 0)");
  LOTUS_CHECK_ARG(C <= 2048, "lotus_softpos_fwd: C = %d > 2048 (W3 is staged in LDS)", C);
  LOTUS_CHECK_ARG((((uintptr_t)h) | ((uintptr_t)w3) | ((uintptr_t)b3) | ((uintptr_t)e)) % 16 == 0,
                  "lotus_softpos_fwd: h, w3, b3 and e must be 16-byte aligned");
  LOTUS_CHECK_ARG(workspace && ((uintptr_t)workspace) % 8 == 0 && workspace_bytes >= lotus_softpos_workspace(B),
                  "lotus_softpos_fwd: workspace too small or misaligned");
  hipStream_t st = (hipStream_t)stream;
  StopEventOnLast stop_ev;
  LOTUS_LAUNCH(softpos_part_kernel, dim3(SP_SPLITS, B), dim3(256), (size_t)4 * C * sizeof(float), st, h, w3, b3, pc, ld, off, C,
               1.0 / temp, e, (double*)workspace);
  stop_ev.last();
  LOTUS_LAUNCH(softpos_merge_kernel, dim3(B), dim3(64), 0, st, (const double*)workspace, xt, stats);
  LOTUS_LAUNCH_CHECK("lotus_softpos_fwd");
  return LOTUS_OK;
}

int lotus_softpos_bwd(const float* g, const float* e, const float* pc, long ld, const int* batch, const double* stats,
                      const float* xt, int B, int n, double temp, float* de, void* stream) {
  LOTUS_CHECK_ARG(g && e && pc && batch && stats && xt && de && B > 0 && n > 0 && ld >= 3 && temp > 0.0,
                  "lotus_softpos_bwd: bad arguments");
  LOTUS_CHECK_ARG((((uintptr_t)e) | ((uintptr_t)de)) % 16 == 0, "lotus_softpos_bwd: e and de must be 16-byte aligned");
  LOTUS_LAUNCH(softpos_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, g, e, pc, ld, batch, stats, xt, n,
               1.0 / temp, de);
  LOTUS_LAUNCH_CHECK("lotus_softpos_bwd");
  return LOTUS_OK;
}

int lotus_reg_loss_fwd(const float* ae, const float* gt, const float* xt, const float* ce, int ce_ld, int B, int W, int ga,
                       int rot_kind, int nrot, float pos_w, float rot_w, float* losses, float* dae, float* dpos, float* xr,
                       void* stream) {
  LOTUS_CHECK_ARG(ae && B > 0 && W >= 2 && rot_kind >= 0 && rot_kind <= 2, "lotus_reg_loss_fwd: bad arguments");
  LOTUS_CHECK_ARG(rot_kind != 0 || (nrot > 0 && W == nrot * 3 + 1), "lotus_reg_loss_fwd: euler_disc takes W == nrot * 3 + 1");
  LOTUS_CHECK_ARG(rot_kind != 1 || W >= 4, "lotus_reg_loss_fwd: euler takes W >= 4 (3 angles + openness)");
  LOTUS_CHECK_ARG(rot_kind != 2 || (W >= 5 && xr), "lotus_reg_loss_fwd: quat takes W >= 5 (4 components + openness) and xr");
  if (gt) {
    LOTUS_CHECK_ARG(losses && dae && dpos && ((xt != nullptr) != (ce != nullptr)) && (!ce || ce_ld > 0),
                    "lotus_reg_loss_fwd: losses need dae, dpos and exactly one of xt / ce");
    LOTUS_CHECK_ARG(ga == (rot_kind == 2 ? 8 : 7), "lotus_reg_loss_fwd: gt has %d columns, rotation kind %d takes %d", ga, rot_kind,
                    rot_kind == 2 ? 8 : 7);
  } else if (rot_kind != 2) {
    return LOTUS_OK;
  }
  RegLossP p;
  p.ae = ae; p.gt = gt; p.xt = xt; p.ce = ce; p.losses = losses; p.dae = dae; p.dpos = dpos; p.xr = xr;
  p.B = B; p.W = W; p.ga = ga; p.rot_kind = rot_kind; p.nrot = nrot; p.ce_ld = ce_ld; p.pos_w = pos_w; p.rot_w = rot_w;
  LOTUS_LAUNCH(reg_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, p);
  LOTUS_LAUNCH_CHECK("lotus_reg_loss_fwd");
  return LOTUS_OK;
}

int lotus_reg_loss_bwd(const float* dae, const float* dpos, const float* gl, float pos_w, float rot_w, int B, int W, float* dae_out,
                       float* dpos_out, void* stream) {
  LOTUS_CHECK_ARG(dae && dpos && gl && dae_out && dpos_out && B > 0 && W >= 2, "lotus_reg_loss_bwd: bad arguments");
  const long nae = (long)B * W, npos = (long)B * 3;
  LOTUS_LAUNCH(reg_loss_bwd_kernel, dim3(cdiv(nae > npos ? nae : npos, 256)), dim3(256), 0, (hipStream_t)stream, dae, dpos, gl,
               pos_w, rot_w, W, nae, npos, dae_out, dpos_out);
  LOTUS_LAUNCH_CHECK("lotus_reg_loss_bwd");
  return LOTUS_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------
// The soft trajectory head of the motion planner (pos_pred_type 'heatmap_mlp' of genrobo3d/models/motion_planner_ptv3.py:
// 55-62,89-109) in two passes.  base = x Wx^T [n][C] is the point-feature part of heatmap_mlp.0, shared by the T steps;
// bias [T][C] carries the step embedding.  Step t, row i:  h_ti = dropout(LeakyReLU(base_i + bias_t)),  e_ti = h_ti W3^T + b3,
// per cloud b:  xt[b][t] = sum_i softmax_i(e_ti0 / temp) (coord_i + e_ti[1:4]).  The hidden layers h_t exist in registers only.
// Dropout: the mask of step t is the one lotus_step_act_fwd makes from splitmix(seed, t) (element index row * C + column), so the
// fused pass computes what lotus_step_act_fwd -> lotus_softpos_fwd compute per step; the T sub-seeds travel by value.
#define MP_TMAX 8     // steps per call (accumulators of every step live in registers)
#define MPB_ROWS 64   // rows per block of the backward pass

struct MpSeeds { unsigned long long s[MP_TMAX]; };

static inline unsigned long long mp_mix(unsigned long long seed, unsigned long long k) {  // == ops.mix_seed (splitmix64 finaliser)
  unsigned long long z = seed + 0x9E3779B97F4A7C15ULL * (k + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

// h (four consecutive channels of one row and step) from the row's base quad x and the step's bias quad s; pre = x + s is kept
__device__ __forceinline__ void mp_hidden4(const float4 x, const float4 s, unsigned long long seed, unsigned long long idx4,
                                           unsigned thresh, float inv_keep, float (&pre)[4], float (&dm)[4], float (&h)[4]) {
  pre[0] = x.x + s.x; pre[1] = x.y + s.y; pre[2] = x.z + s.z; pre[3] = x.w + s.w;
  dm[0] = dm[1] = dm[2] = dm[3] = 1.f;
  if (thresh) dropout_scale4(seed, idx4, thresh, inv_keep, dm);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    h[k] = act_f(pre[k], LOTUS_ACT_LEAKY);
    if (thresh) h[k] *= dm[k];
  }
}

// chunk s of cloud b, all T steps: e_t rows of the chunk, then the chunk's softmax partial of every step
// part [B][T][SP_SPLITS][SP_PART] (the layout softpos_merge_kernel reads with "cloud" = b * T + t)
template <int T>
__global__ __launch_bounds__(256) void mp_softpos_part_kernel(const float* __restrict__ base, const float* __restrict__ bias,
                                                              const float* __restrict__ w3, const float* __restrict__ b3,
                                                              const float* __restrict__ pc, long ld, const int* __restrict__ off,
                                                              int n, int C, double inv_temp, MpSeeds seeds, unsigned thresh,
                                                              float inv_keep, float* __restrict__ e, double* __restrict__ part) {
  LOTUS_T_PRIO();
  extern __shared__ float4 mp_w[];  // W3 [4][C / 4], then the bias rows [T][C / 4]
  __shared__ float red[T][4];
  __shared__ double redd[T][4][4];
  const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n0 = off[b], nn = off[b + 1] - n0;
  const int p0 = n0 + (int)((long)nn * s / SP_SPLITS), p1 = n0 + (int)((long)nn * (s + 1) / SP_SPLITS);
  const int c4 = C / 4;
  if (p0 < p1) {
    for (int i = tid; i < 4 * c4; i += 256) mp_w[i] = ld4q(w3, i);
    for (int i = tid; i < T * c4; i += 256) mp_w[4 * c4 + i] = ld4q(bias, i);
  }
  __syncthreads();
  const int l = tid % SP_LPR, g = tid / SP_LPR;
  const float4 b3v = ld4(b3);
  float m[T];
#pragma unroll
  for (int t = 0; t < T; ++t) m[t] = -INFINITY;
  for (int r0 = p0; r0 < p1; r0 += 256 / SP_LPR) {  // (uniform trip count: the shuffles below see every lane)
    const int row = r0 + g;
    const bool valid = row < p1;
    float a[T][4];
#pragma unroll
    for (int t = 0; t < T; ++t) a[t][0] = a[t][1] = a[t][2] = a[t][3] = 0.f;
    if (valid) {
      const float* hr = base + (long)row * C;
      for (int q = l; q < c4; q += SP_LPR) {
        const float4 x = ld4q(hr, q);
        const float4 u0 = mp_w[q], u1 = mp_w[c4 + q], u2 = mp_w[2 * c4 + q], u3 = mp_w[3 * c4 + q];
        const unsigned long long idx4 = (unsigned long long)((long)row * C + 4 * q);
#pragma unroll
        for (int t = 0; t < T; ++t) {
          float pre[4], dm[4], h[4];
          mp_hidden4(x, mp_w[(4 + t) * c4 + q], seeds.s[t], idx4, thresh, inv_keep, pre, dm, h);
          a[t][0] = fmaf(h[0], u0.x, fmaf(h[1], u0.y, fmaf(h[2], u0.z, fmaf(h[3], u0.w, a[t][0]))));
          a[t][1] = fmaf(h[0], u1.x, fmaf(h[1], u1.y, fmaf(h[2], u1.z, fmaf(h[3], u1.w, a[t][1]))));
          a[t][2] = fmaf(h[0], u2.x, fmaf(h[1], u2.y, fmaf(h[2], u2.z, fmaf(h[3], u2.w, a[t][2]))));
          a[t][3] = fmaf(h[0], u3.x, fmaf(h[1], u3.y, fmaf(h[2], u3.z, fmaf(h[3], u3.w, a[t][3]))));
        }
      }
    }
#pragma unroll
    for (int o = SP_LPR >> 1; o > 0; o >>= 1) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        a[t][0] += __shfl_xor(a[t][0], o, 64); a[t][1] += __shfl_xor(a[t][1], o, 64);
        a[t][2] += __shfl_xor(a[t][2], o, 64); a[t][3] += __shfl_xor(a[t][3], o, 64);
      }
    }
    if (valid && l == 0) {
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float a0 = a[t][0] + b3v.x;
        st4(e + ((long)t * n + row) * 4, make_float4(a0, a[t][1] + b3v.y, a[t][2] + b3v.z, a[t][3] + b3v.w));
        m[t] = fmaxf(m[t], a0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const float w = wave_max(m[t]);
    if ((tid & 63) == 0) red[t][tid >> 6] = w;
  }
  __syncthreads();  // (also orders the e rows written above before the reads below: same block)
  double zm[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    zm[t] = (double)fmaxf(fmaxf(red[t][0], red[t][1]), fmaxf(red[t][2], red[t][3])) * inv_temp;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int row = p0 + tid; row < p1; row += 256) {
      const float4 er = ld4(e + ((long)t * n + row) * 4);
      const float* cr = pc + (long)row * ld;
      const double w = exp((double)er.x * inv_temp - zm[t]);
      v[0] += w;
      v[1] += w * ((double)cr[0] + (double)er.y);
      v[2] += w * ((double)cr[1] + (double)er.z);
      v[3] += w * ((double)cr[2] + (double)er.w);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double w = reg_wave_sum_d(v[k]);
      if ((tid & 63) == 0) redd[t][k][tid >> 6] = w;
    }
  }
  __syncthreads();
  if (tid < T) {
    const int t = tid;
    double* o = part + (((long)b * T + t) * SP_SPLITS + s) * SP_PART;
    double z = -INFINITY;
#pragma unroll
    for (int u = 0; u < T; ++u) if (u == t) z = zm[u];
    o[0] = p0 < p1 ? z : -INFINITY;
    for (int k = 0; k < 4; ++k) o[1 + k] = ((redd[t][k][0] + redd[t][k][1]) + redd[t][k][2]) + redd[t][k][3];
  }
}

struct MpBwdP {
  const float* g; const float* base; const float* bias; const float* w3; const float* e; const float* pc;
  const int* batch; const double* stats; const float* xt;
  float* dbase; float* part;
  long ld, part_stride;
  double inv_temp;
  MpSeeds seeds;
  int n, C;
  unsigned thresh;
  float inv_keep;
};

// rows [blockIdx.x * MPB_ROWS, + MPB_ROWS): de_t of every (row, step) into LDS (as softpos_bwd_kernel forms it), then one sweep
// over the block's base rows, 64 channels at a time: h_t and the mask are regenerated, dpre_t = (de_t W3) mask act'(pre_t),
// dbase = sum_t dpre_t is stored once, and the column sums  dbias_t = sum_i dpre_ti,  dw3[k] = sum_t sum_i de_tik h_ti  and
// db3[k] = sum_t sum_i de_tik  go to the block's slot of part ([T][C] | [4][C] | [4]) for the fixed-order reduction.
template <int T>
__global__ __launch_bounds__(256) void mp_softpos_bwd_kernel(MpBwdP p) {
  LOTUS_T_PRIO();
  __shared__ float4 de_s[MPB_ROWS * T];
  __shared__ float4 red[4][T + 4][SP_LPR];
  __shared__ double redd[4][4];
  const int tid = threadIdx.x, n = p.n, C = p.C, c4 = C / 4;
  const int r0 = blockIdx.x * MPB_ROWS, nr = min(MPB_ROWS, n - r0);
  float* part = p.part + (long)blockIdx.x * p.part_stride;
  double s4[4] = {0.0, 0.0, 0.0, 0.0};
  for (int idx = tid; idx < nr * T; idx += 256) {
    const int r = idx / T, t = idx % T, row = r0 + r;
    const int bt = p.batch[row] * T + t;
    const float4 er = ld4(p.e + ((long)t * n + row) * 4);
    const float* cr = p.pc + (long)row * p.ld;
    const double pr = exp((double)er.x * p.inv_temp - p.stats[bt * 2 + 1]);
    const double g0 = p.g[bt * 3], g1 = p.g[bt * 3 + 1], g2 = p.g[bt * 3 + 2];
    // q_i is rounded to the precision xt is stored in before the difference: a cloud of one point (p = 1, xt = q) then has
    // q - xt == 0, hence de_0 == 0, exactly
    const double d0 = (double)(float)((double)cr[0] + (double)er.y) - (double)p.xt[bt * 3];
    const double d1 = (double)(float)((double)cr[1] + (double)er.z) - (double)p.xt[bt * 3 + 1];
    const double d2 = (double)(float)((double)cr[2] + (double)er.w) - (double)p.xt[bt * 3 + 2];
    const float4 de = make_float4((float)(pr * (d0 * g0 + d1 * g1 + d2 * g2) * p.inv_temp), (float)(pr * g0), (float)(pr * g1),
                                  (float)(pr * g2));
    de_s[idx] = de;
    s4[0] += (double)de.x; s4[1] += (double)de.y; s4[2] += (double)de.z; s4[3] += (double)de.w;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double w = reg_wave_sum_d(s4[k]);
    if ((tid & 63) == 0) redd[k][tid >> 6] = w;
  }
  __syncthreads();
  if (tid < 4) part[(long)(T + 4) * C + tid] = (float)(((redd[tid][0] + redd[tid][1]) + redd[tid][2]) + redd[tid][3]);
  const int l = tid % SP_LPR, g = tid / SP_LPR, wv = tid >> 6;
  for (int j = 0; j < (c4 + SP_LPR - 1) / SP_LPR; ++j) {  // (uniform trip count: shuffles and barriers below see every lane)
    const int q = l + j * SP_LPR;
    const bool vq = q < c4;
    float4 u[4], sb[T], ab[T], aw[4];
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 4; ++k) { u[k] = vq ? ld4q(p.w3 + (long)k * C, q) : zero; aw[k] = zero; }
#pragma unroll
    for (int t = 0; t < T; ++t) { sb[t] = vq ? ld4q(p.bias + (long)t * C, q) : zero; ab[t] = zero; }
    for (int rr = g; rr < MPB_ROWS; rr += 256 / SP_LPR) {
      if (!vq || rr >= nr) continue;
      const int row = r0 + rr;
      const float4 x = ld4q(p.base + (long)row * C, q);
      const unsigned long long idx4 = (unsigned long long)((long)row * C + 4 * q);
      float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const float4 de = de_s[rr * T + t];
        float pre[4], dm[4], h[4];
        mp_hidden4(x, sb[t], p.seeds.s[t], idx4, p.thresh, p.inv_keep, pre, dm, h);
        aw[0].x += de.x * h[0]; aw[0].y += de.x * h[1]; aw[0].z += de.x * h[2]; aw[0].w += de.x * h[3];
        aw[1].x += de.y * h[0]; aw[1].y += de.y * h[1]; aw[1].z += de.y * h[2]; aw[1].w += de.y * h[3];
        aw[2].x += de.z * h[0]; aw[2].y += de.z * h[1]; aw[2].z += de.z * h[2]; aw[2].w += de.z * h[3];
        aw[3].x += de.w * h[0]; aw[3].y += de.w * h[1]; aw[3].z += de.w * h[2]; aw[3].w += de.w * h[3];
        const float dh[4] = {fmaf(de.x, u[0].x, fmaf(de.y, u[1].x, fmaf(de.z, u[2].x, de.w * u[3].x))),
                             fmaf(de.x, u[0].y, fmaf(de.y, u[1].y, fmaf(de.z, u[2].y, de.w * u[3].y))),
                             fmaf(de.x, u[0].z, fmaf(de.y, u[1].z, fmaf(de.z, u[2].z, de.w * u[3].z))),
                             fmaf(de.x, u[0].w, fmaf(de.y, u[1].w, fmaf(de.z, u[2].w, de.w * u[3].w)))};
        float d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          d[k] = dh[k] * act_grad_f(pre[k], LOTUS_ACT_LEAKY) * dm[k];
          o[k] += d[k];
        }
        ab[t].x += d[0]; ab[t].y += d[1]; ab[t].z += d[2]; ab[t].w += d[3];
      }
      st4q(p.dbase + (long)row * C, q, make_float4(o[0], o[1], o[2], o[3]));
    }
    // column sums: the four row groups of a wave by shuffle, the four waves through LDS in fixed order
#pragma unroll
    for (int sl = 0; sl < T + 4; ++sl) {
      float4 v = sl < T ? ab[sl < T ? sl : 0] : aw[sl < T ? 0 : sl - T];
#pragma unroll
      for (int o = SP_LPR; o < 64; o <<= 1) {
        v.x += __shfl_xor(v.x, o, 64); v.y += __shfl_xor(v.y, o, 64); v.z += __shfl_xor(v.z, o, 64); v.w += __shfl_xor(v.w, o, 64);
      }
      if ((tid & 63) < SP_LPR) red[wv][sl][l] = v;
    }
    __syncthreads();
    if (tid < (T + 4) * SP_LPR && vq) {  // (tid / SP_LPR = slot, tid % SP_LPR = l: q is this thread's own quad)
      const int sl = tid / SP_LPR;
      float4 v = red[0][sl][l];
      for (int w = 1; w < 4; ++w) {
        const float4 r = red[w][sl][l];
        v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
      }
      st4q(part + (long)sl * C, q, v);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Trajectory losses with the soft position (motion_planner_ptv3.py:338-397, pos_pred_type 'heatmap_mlp', rot_pred_type
// 'euler_disc'): one block, double arithmetic, fixed-order sums.  Row r = b * T + t; ae [B*T][W], W = nrot * 3 + 2 (rotation
// logits (bin, axis) at bin * 3 + axis | openness | stop); gt [B*T][ga] (position 0..2, rotation bins 3..5, openness ga-1).
//   pos = sum_r mask_r |xt_r - gt_r[0:3]|^2 / sum mask / 3  (one global normalisation, :340-342)   rot, open, stop: as mp_loss_kernel
// dae / dxt keep the partial derivatives of the loss each column belongs to; rows with mask 0 get exact zeros.
__global__ __launch_bounds__(256) void mp_reg_loss_kernel(const float* __restrict__ ae, const float* __restrict__ gt,
                                                          const float* __restrict__ stop, const float* __restrict__ mask,
                                                          const float* __restrict__ xt, int R, int nrot, int ga, float pos_w,
                                                          float rot_w, float* __restrict__ losses, float* __restrict__ dae,
                                                          float* __restrict__ dxt) {
  LOTUS_T_PRIO();
  __shared__ double red[4][4];
  __shared__ double msum_s;
  const int W = nrot * 3 + 2, tid = threadIdx.x;
  double ms = 0.0;
  for (int r = tid; r < R; r += 256) ms += (double)mask[r];
  ms = reg_wave_sum_d(ms);
  if ((tid & 63) == 0) red[0][tid >> 6] = ms;
  __syncthreads();
  if (tid == 0) msum_s = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
  __syncthreads();
  const double msum = msum_s;
  double pos = 0.0, rot = 0.0, opn = 0.0, stp = 0.0;
  for (int i = tid; i < R * 3; i += 256) {
    const int r = i / 3, a = i % 3;
    const double m = mask[r];
    const float* row = ae + (long)r * W;
    float mx = -INFINITY;
    for (int k = 0; k < nrot; ++k) mx = fmaxf(mx, row[k * 3 + a]);
    double se = 0.0;
    for (int k = 0; k < nrot; ++k) se += exp((double)row[k * 3 + a] - (double)mx);
    const double lse = (double)mx + log(se);
    const int tk = min(max((int)gt[(long)r * ga + 3 + a], 0), nrot - 1);
    rot += (lse - (double)row[tk * 3 + a]) * m;
    const double sc = m / msum / 3.0;
    for (int k = 0; k < nrot; ++k)
      dae[(long)r * W + k * 3 + a] = (float)((exp((double)row[k * 3 + a] - lse) - (k == tk ? 1.0 : 0.0)) * sc);
    const double d = (double)xt[i] - (double)gt[(long)r * ga + a];
    pos += d * d * m;
    dxt[i] = (float)(2.0 * d * sc);
  }
  for (int r = tid; r < R; r += 256) {
    const double m = mask[r], sc = m / msum;
    const double xo = ae[(long)r * W + W - 2], to = gt[(long)r * ga + ga - 1];
    opn += (fmax(xo, 0.0) - xo * to + log1p(exp(-fabs(xo)))) * m;
    dae[(long)r * W + W - 2] = (float)((1.0 / (1.0 + exp(-xo)) - to) * sc);
    const double xs = ae[(long)r * W + W - 1], ts = stop[r];
    stp += (fmax(xs, 0.0) - xs * ts + log1p(exp(-fabs(xs)))) * m;
    dae[(long)r * W + W - 1] = (float)((1.0 / (1.0 + exp(-xs)) - ts) * sc);
  }
  const double v4[4] = {pos, rot, opn, stp};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double w = reg_wave_sum_d(v4[k]);
    if ((tid & 63) == 0) red[k][tid >> 6] = w;
  }
  __syncthreads();
  if (tid == 0) {
    double t4[4];
    for (int k = 0; k < 4; ++k) t4[k] = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
    const double lp = t4[0] / msum / 3.0, lr = t4[1] / msum / 3.0, lo = t4[2] / msum, ls = t4[3] / msum;
    losses[0] = (float)lp; losses[1] = (float)lr; losses[2] = (float)lo; losses[3] = (float)ls;
    losses[4] = (float)((double)pos_w * lp + (double)rot_w * lr + lo + ls);
  }
}

// upstream gradient gl[5] (device) of the five losses -> d ae [B*T][W], d xt [B*T][3]
__global__ void mp_reg_loss_bwd_kernel(const float* __restrict__ dae, const float* __restrict__ dxt, const float* __restrict__ gl,
                                       float pos_w, float rot_w, int W, long nae, long nxt, float* __restrict__ dae_out,
                                       float* __restrict__ dxt_out) {
  LOTUS_T_PRIO();
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nae) {
    const int col = (int)(i % W);
    dae_out[i] = dae[i] * (col == W - 1 ? gl[3] + gl[4] : col == W - 2 ? gl[2] + gl[4] : gl[1] + rot_w * gl[4]);
  }
  if (i < nxt) dxt_out[i] = dxt[i] * (gl[0] + pos_w * gl[4]);
}

int lotus_reduce_parts(const float* part, float* out, long n, long stride, int nz, int accumulate, hipStream_t st);  // gemm.hip

#define MP_DISPATCH_T(T_, ...)                                                       \
  switch (T_) {                                                                      \
    case 1: { constexpr int TT = 1; __VA_ARGS__; } break;                            \
    case 2: { constexpr int TT = 2; __VA_ARGS__; } break;                            \
    case 3: { constexpr int TT = 3; __VA_ARGS__; } break;                            \
    case 4: { constexpr int TT = 4; __VA_ARGS__; } break;                            \
    case 5: { constexpr int TT = 5; __VA_ARGS__; } break;                            \
    case 6: { constexpr int TT = 6; __VA_ARGS__; } break;                            \
    case 7: { constexpr int TT = 7; __VA_ARGS__; } break;                            \
    default: { constexpr int TT = 8; __VA_ARGS__; } break;                           \
  }

static size_t mp_bwd_part_stride(int C, int T) { return (size_t)(T + 4) * C + 4; }  // [T][C] dbias | [4][C] dw3 | [4] db3

extern "C" {

size_t lotus_mp_softpos_workspace(int B, int T) {
  return (size_t)(B > 0 ? B : 1) * (T > 0 ? T : 1) * SP_SPLITS * SP_PART * sizeof(double);
}

size_t lotus_mp_softpos_bwd_workspace(int n, int C, int T) {
  return (size_t)cdiv(n > 0 ? n : 1, MPB_ROWS) * mp_bwd_part_stride(C > 0 ? C : 4, T > 0 ? T : 1) * sizeof(float);
}

int lotus_mp_softpos_fwd(const float* base, const float* bias, const float* w3, const float* b3, const float* pc, long ld,
                         const int* off, int B, int n, int C, int T, double temp, float drop_p, unsigned long long seed, float* e,
                         float* xt, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
  LOTUS_CHECK_ARG(base && bias && w3 && b3 && pc && off && e && xt && stats, "lotus_mp_softpos_fwd: null pointer");
  LOTUS_CHECK_ARG(B > 0 && n > 0 && T > 0, "lotus_mp_softpos_fwd: B = %d, n = %d, T = %d must be positive", B, n, T);
  LOTUS_CHECK_ARG(T <= MP_TMAX, "lotus_mp_softpos_fwd: T = %d > %d steps", T, MP_TMAX);
  LOTUS_CHECK_ARG(C >= 4 && C % 4 == 0 && C <= 2048, "lotus_mp_softpos_fwd: C = %d (4 <= C <= 2048, C %% 4 == 0: W3 and the bias rows are staged in LDS)", C);
  LOTUS_CHECK_ARG(ld >= 3, "lotus_mp_softpos_fwd: ld = %ld < 3", ld);
  LOTUS_CHECK_ARG(temp > 0.0, "lotus_mp_softpos_fwd: temp must be > 0");
  LOTUS_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "lotus_mp_softpos_fwd: drop_p outside [0, 1)");
  LOTUS_CHECK_ARG((((uintptr_t)base) | ((uintptr_t)bias) | ((uintptr_t)w3) | ((uintptr_t)b3) | ((uintptr_t)e)) % 16 == 0,
                  "lotus_mp_softpos_fwd: base, bias, w3, b3 and e must be 16-byte aligned");
  LOTUS_CHECK_ARG(workspace && ((uintptr_t)workspace) % 8 == 0 && workspace_bytes >= lotus_mp_softpos_workspace(B, T),
                  "lotus_mp_softpos_fwd: workspace too small or misaligned");
  hipStream_t st = (hipStream_t)stream;
  MpSeeds seeds;
  for (int t = 0; t < MP_TMAX; ++t) seeds.s[t] = mp_mix(seed, (unsigned long long)t);
  unsigned th; float inv;
  lotus_drop_setup(drop_p, &th, &inv);
  const size_t lds = (size_t)(4 + T) * C * sizeof(float);
  StopEventOnLast stop_ev;
  MP_DISPATCH_T(T, {
    if (lds > 65536 && hipFuncSetAttribute((const void*)mp_softpos_part_kernel<TT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds) != hipSuccess) {
      (void)hipGetLastError();
      lotus_set_error("lotus_mp_softpos_fwd: launch failed: %zu bytes of LDS refused", lds);
      return LOTUS_E_LAUNCH;
    }
    LOTUS_LAUNCH(mp_softpos_part_kernel<TT>, dim3(SP_SPLITS, B), dim3(256), lds, st, base, bias, w3, b3, pc, ld, off, n, C,
                 1.0 / temp, seeds, th, inv, e, (double*)workspace);
  });
  stop_ev.last();
  LOTUS_LAUNCH(softpos_merge_kernel, dim3(B * T), dim3(64), 0, st, (const double*)workspace, xt, stats);
  LOTUS_LAUNCH_CHECK("lotus_mp_softpos_fwd");
  return LOTUS_OK;
}

int lotus_mp_softpos_bwd(const float* g, const float* base, const float* bias, const float* w3, const float* e, const float* pc,
                         long ld, const int* batch, const double* stats, const float* xt, int B, int n, int C, int T, double temp,
                         float drop_p, unsigned long long seed, float* dbase, float* dbias, float* dw3, float* db3,
                         void* workspace, size_t workspace_bytes, void* stream) {
  LOTUS_CHECK_ARG(g && base && bias && w3 && e && pc && batch && stats && xt && dbase && dbias && dw3 && db3,
                  "lotus_mp_softpos_bwd: null pointer");
  LOTUS_CHECK_ARG(B > 0 && n > 0 && T > 0, "lotus_mp_softpos_bwd: B = %d, n = %d, T = %d must be positive", B, n, T);
  LOTUS_CHECK_ARG(T <= MP_TMAX, "lotus_mp_softpos_bwd: T = %d > %d steps", T, MP_TMAX);
  LOTUS_CHECK_ARG(C >= 4 && C % 4 == 0 && C <= 2048, "lotus_mp_softpos_bwd: C = %d (4 <= C <= 2048, C %% 4 == 0)", C);
  LOTUS_CHECK_ARG(ld >= 3, "lotus_mp_softpos_bwd: ld = %ld < 3", ld);
  LOTUS_CHECK_ARG(temp > 0.0, "lotus_mp_softpos_bwd: temp must be > 0");
  LOTUS_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "lotus_mp_softpos_bwd: drop_p outside [0, 1)");
  LOTUS_CHECK_ARG((((uintptr_t)base) | ((uintptr_t)bias) | ((uintptr_t)w3) | ((uintptr_t)e) | ((uintptr_t)dbase)) % 16 == 0,
                  "lotus_mp_softpos_bwd: base, bias, w3, e and dbase must be 16-byte aligned");
  LOTUS_CHECK_ARG(workspace && ((uintptr_t)workspace) % 16 == 0 && workspace_bytes >= lotus_mp_softpos_bwd_workspace(n, C, T),
                  "lotus_mp_softpos_bwd: workspace too small or misaligned");
  hipStream_t st = (hipStream_t)stream;
  MpBwdP p;
  p.g = g; p.base = base; p.bias = bias; p.w3 = w3; p.e = e; p.pc = pc; p.batch = batch; p.stats = stats; p.xt = xt;
  p.dbase = dbase; p.part = (float*)workspace; p.ld = ld; p.part_stride = (long)mp_bwd_part_stride(C, T);
  p.inv_temp = 1.0 / temp; p.n = n; p.C = C;
  for (int t = 0; t < MP_TMAX; ++t) p.seeds.s[t] = mp_mix(seed, (unsigned long long)t);
  lotus_drop_setup(drop_p, &p.thresh, &p.inv_keep);
  const int nb = cdiv(n, MPB_ROWS);
  StopEventOnLast stop_ev;
  MP_DISPATCH_T(T, LOTUS_LAUNCH(mp_softpos_bwd_kernel<TT>, dim3(nb), dim3(256), 0, st, p));
  LOTUS_LAUNCH_CHECK("lotus_mp_softpos_bwd");
  const float* part = (const float*)workspace;
  int rc = lotus_reduce_parts(part, dbias, (long)T * C, p.part_stride, nb, 0, st);
  if (!rc) rc = lotus_reduce_parts(part + (long)T * C, dw3, 4L * C, p.part_stride, nb, 0, st);
  stop_ev.last();
  if (!rc) rc = lotus_reduce_parts(part + (long)(T + 4) * C, db3, 4, p.part_stride, nb, 0, st);
  return rc;
}

int lotus_mp_reg_loss_fwd(const float* ae, const float* gt, const float* stop, const float* mask, const float* xt, int B, int T,
                          int nrot, int ga, float pos_w, float rot_w, float* losses, float* dae, float* dxt, void* stream) {
  LOTUS_CHECK_ARG(ae && gt && stop && mask && xt && losses && dae && dxt, "lotus_mp_reg_loss_fwd: null pointer");
  LOTUS_CHECK_ARG(B > 0 && T > 0 && nrot > 0 && ga >= 7 && (long)B * T * 3 < (1L << 31),
                  "lotus_mp_reg_loss_fwd: bad arguments (B, T, nrot > 0, gt has >= 7 columns)");
  LOTUS_LAUNCH(mp_reg_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ae, gt, stop, mask, xt, B * T, nrot, ga, pos_w, rot_w,
               losses, dae, dxt);
  LOTUS_LAUNCH_CHECK("lotus_mp_reg_loss_fwd");
  return LOTUS_OK;
}

int lotus_mp_reg_loss_bwd(const float* dae, const float* dxt, const float* gl, float pos_w, float rot_w, int B, int T, int nrot,
                          float* dae_out, float* dxt_out, void* stream) {
  LOTUS_CHECK_ARG(dae && dxt && gl && dae_out && dxt_out, "lotus_mp_reg_loss_bwd: null pointer");
  LOTUS_CHECK_ARG(B > 0 && T > 0 && nrot > 0, "lotus_mp_reg_loss_bwd: bad arguments (B, T, nrot > 0)");
  const int W = nrot * 3 + 2;
  const long nae = (long)B * T * W, nxt = (long)B * T * 3;
  LOTUS_LAUNCH(mp_reg_loss_bwd_kernel, dim3(cdiv(nae, 256)), dim3(256), 0, (hipStream_t)stream, dae, dxt, gl, pos_w, rot_w, W, nae,
               nxt, dae_out, dxt_out);
  LOTUS_LAUNCH_CHECK("lotus_mp_reg_loss_bwd");
  return LOTUS_OK;
}

}  // extern "C"

}  // namespace LOTUS_NS
