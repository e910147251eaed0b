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

}  // namespace LOTUS_NS
