// lotus-hip: patch attention with the relative-position term of SerializedAttention (PointTransformerV3/model.py:307-326 RPE,
// :400-408, :518-527: the non-flash branch with enable_rpe).  Before the softmax the score of query row i and key row j of a patch,
// head h, gets
//   bias(i, j, h) = sum_{a in x, y, z} table[a * num + clamp(g_i[a] - g_j[a], -bnd, bnd) + bnd][h],   num = 2 bnd + 1
// with g the level's integer grid coordinate of the row (borrowed rows included); the term is NOT multiplied by the softmax scale.
// The scores never leave the kernel, so the term cannot be a pass of its own: these are the exact-fp32 128 x 128 tile kernels of
// attention.hip (family 1 forward at precision 0, family 3 backward; that file is not touched, what both need — the row loads, the
// per-row LayerNorm, the dropout hash with its element numbering, the fix-up of borrowed rows and the reduction of the norm
// partials — is restated here) with
//   forward   the head's table column (<= 93 floats) and the tile's grid rows in LDS; a lane owns one query, keeps its three
//             coordinates in registers and adds three LDS lookups to each of its 64 scores after the scale;
//   backward  the same three lookups (in log2 units) on the recomputed scores; the gradient of the table is the sum of
//             G = P o (dP - delta) (dropout mask applied as for dS, NOT times the scale) over every pair that selects a table row.
// The table gradient has no atomics.  In the backward kernel a lane owns one key and its registers run over the queries: every key
// has a private row of 3 num fp32 bins in LDS.  The lower lane half of a wave adds its own sixteen values of a query tile and then
// the sixteen of its partner lane (same key, lane ^ 32, handed over by shuffle) in program order, over all query tiles and all
// tiles of the block; at the end of the block the bins of the <= 128 keys are summed in ascending key order in float64 into one
// partial row per (block, head), and a merge kernel sums the partial rows in ascending block order in float64.  Every order is
// fixed: reruns are bit-identical.  Rows that no pair selects only ever receive nothing: they are written as exact zeros.
// fp32 storage only (no bf16 twin).
#include "mma.h"
#include "attn_route.h"

namespace LOTUS_NS {

#define RT 128           // tile rows (queries) and max keys
#define RLD 33           // row stride of the [128][d <= 32] images
#define RPE_MAX_BND 15   // pos_bnd of the largest patch the tile kernels take: int((4 * 128) ** (1 / 3) * 2)
#define RPE_MAX_ROWS 96  // >= 3 (2 RPE_MAX_BND + 1) = 93, a multiple of 4
#define RPE_LOG2E 1.4426950408889634f

struct RpeP {
  const float* q; long q_ld; int q_off;
  const float* kv; long kv_ld; int k_off, v_off;
  const int* qidx; const int* kidx; const int* owner;
  const int* tiles;   // [ntiles][4] = q_start, q_len, k_start, k_len
  const int* blocks;  // bwd: [nblocks][6] = first_tile, n_tiles, tile_step, part_slot, k_start, k_len
  const float* qn_w; const float* qn_b; const float* kn_w; const float* kn_b;
  float* out; long out_ld;
  float* lse;  // [npos][H]
  const float* dout;
  float* dq; long dq_ld; int dq_off;
  float* dkv; long dkv_ld; int dk_off, dv_off; long dkv_part_stride;
  float* ln_part;    // [nblocks * H][4][32]  dgamma_q, dbeta_q, dgamma_k, dbeta_k
  double* tab_part;  // [nblocks * H][3 num]
  const int* kext; float* dkv_extra; long dkv_extra_ld;
  const int* grid;     // [n][3]
  const float* table;  // [3 num][H]
  int bnd;
  int H, d;
  float scale, eps;
  unsigned long long drop_seed;
  unsigned drop_thresh;
  float drop_inv_keep;
};

// dropout on the probabilities: the function and the element numbering of attention.hip (keep_lo there) —
// idx = ((tile * H + h) * 128 + q) * 128 + key, keep iff mix(seed, idx) >= thresh
__device__ __forceinline__ bool rpe_keep_lo(unsigned lo, unsigned s0, unsigned c2, unsigned thresh) {
  unsigned x = lo * 0x9E3779B1u + s0;
  x ^= c2;
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15;
  return x >= thresh;
}

__device__ __forceinline__ f32x16 rpe_zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

struct RpeRowSrc {
  float* img;
  const float* base;
  long ld;
  int coff;
  const int* rows_s;
  int len;
};
// `len` gathered rows of d floats into img[128][RLD], rows >= len and columns >= d zero; every global load is issued before the
// first LDS store
template <int N>
__device__ __forceinline__ void rpe_load_rows(const RpeRowSrc (&src)[N], int d) {
  const int sub = threadIdx.x & 7, r0 = threadIdx.x >> 3;
  float4 v[N][4];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = r0 + 32 * j;
      v[i][j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < src[i].len && sub * 4 < d)
        v[i][j] = ld4(src[i].base + (long)src[i].rows_s[r] * src[i].ld + src[i].coff + sub * 4);
    }
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float* o = src[i].img + (r0 + 32 * j) * RLD + sub * 4;
      o[0] = v[i][j].x; o[1] = v[i][j].y; o[2] = v[i][j].z; o[3] = v[i][j].w;
    }
}

template <bool AFFINE>
__device__ __forceinline__ void rpe_ln_rows(float* img, float* rstd_s, int row, int len, int d, float eps, const float* g_s,
                                            const float* b_s) {
  if (row >= len) {
    if (row < RT) rstd_s[row] = 0.f;
    return;
  }
  float* x = img + row * RLD;
  float m = 0.f;
  for (int j = 0; j < d; ++j) m += x[j];
  m /= d;
  float v = 0.f;
  for (int j = 0; j < d; ++j) {
    const float c = x[j] - m;
    v += c * c;
  }
  const float rs = rsqrtf(v / d + eps);
  rstd_s[row] = rs;
  for (int j = 0; j < d; ++j) {
    const float xh = (x[j] - m) * rs;
    x[j] = AFFINE ? xh * g_s[j] + b_s[j] : xh;
  }
}

__device__ __forceinline__ void rpe_ln_rows_bwd(float* g, const float* xh, const float* rstd_s, int row, int len, int d,
                                                const float* gam) {
  if (row >= len) return;
  float* gr = g + row * RLD;
  const float* xr = xh + row * RLD;
  float s1 = 0.f, s2 = 0.f;
  for (int j = 0; j < d; ++j) {
    const float t = gr[j] * gam[j];
    s1 += t;
    s2 += t * xr[j];
  }
  s1 /= d;
  s2 /= d;
  const float rs = rstd_s[row];
  for (int j = 0; j < d; ++j) gr[j] = rs * (gr[j] * gam[j] - s1 - xr[j] * s2);
}

// plain stores: one owner per row; a borrowed key row (ext_s[r] >= 0) goes to its row of the side buffer
__device__ __forceinline__ void rpe_store_rows(const float* img, float* base, long ld, int coff, const int* rows_s, const int* own_s,
                                               int len, int d, const int* ext_s = nullptr, float* ext_base = nullptr,
                                               long ext_ld = 0, int ext_coff = 0) {
  const int sub = threadIdx.x & 7;
  for (int r = threadIdx.x >> 3; r < len; r += 32) {
    if (own_s && !own_s[r]) continue;
    if (sub * 4 >= d) continue;
    const float* v = img + r * RLD + sub * 4;
    float* o = base + (long)rows_s[r] * ld + coff + sub * 4;
    if (ext_s && ext_s[r] >= 0) o = ext_base + (long)ext_s[r] * ext_ld + ext_coff + sub * 4;
    st4(o, make_float4(v[0], v[1], v[2], v[3]));
  }
}

// the LDS of both kernels (floats unless noted): row images, per-row scalars, the norm's affine vectors, the row tables, the
// head's table column, the grid rows of the tile's queries (forward: and keys), backward only the per-key bins
struct RpeSmem {
  float* Q; float* K; float* V; float* dO;
  float* qrstd; float* krstd; float* Dv; float* lse;
  float* gq; float* bq; float* gk; float* bk;
  int* qrow; int* krow; int* qown; int* kext;
  float* tab; int* qg; int* kg; float* bins;
};
__device__ __forceinline__ RpeSmem rpe_carve(float* base, bool bwd) {
  RpeSmem s;
  float* p = base;
  s.Q = p; p += RT * RLD;
  s.K = p; p += RT * RLD;
  s.V = p; p += RT * RLD;
  s.dO = p; if (bwd) p += RT * RLD;
  s.qrstd = p; p += RT;
  s.krstd = p; p += RT;
  s.Dv = p; if (bwd) p += RT;
  s.lse = p; if (bwd) p += RT;
  s.gq = p; p += 32; s.bq = p; p += 32; s.gk = p; p += 32; s.bk = p; p += 32;
  s.qrow = (int*)p; p += RT;
  s.krow = (int*)p; p += RT;
  s.qown = (int*)p; p += RT;
  s.kext = (int*)p; if (bwd) p += RT;
  s.tab = p; p += RPE_MAX_ROWS;
  s.qg = (int*)p; p += 3 * RT;
  s.kg = (int*)p; if (!bwd) p += 3 * RT;
  s.bins = p;
  return s;
}
static size_t rpe_smem_bytes(bool bwd, int bnd) {
  const size_t rows = 3 * (2 * (size_t)bnd + 1);
  return ((bwd ? 4 : 3) * RT * RLD + (bwd ? 4 : 2) * RT + 4 * 32 + (bwd ? 4 : 3) * RT + RPE_MAX_ROWS + (bwd ? 3 : 6) * RT +
          (bwd ? RT * rows : 0)) * sizeof(float);
}

__device__ __forceinline__ void rpe_load_affine(const RpeP& p, RpeSmem& s) {
  const int t = threadIdx.x;
  if (t < 32) {
    const bool in = t < p.d;
    s.gq[t] = in ? p.qn_w[t] : 0.f;
    s.bq[t] = in ? p.qn_b[t] : 0.f;
    s.gk[t] = in ? p.kn_w[t] : 0.f;
    s.bk[t] = in ? p.kn_b[t] : 0.f;
  }
}

__device__ __forceinline__ int rpe_bin(int gq, int gk, int bnd) { return min(max(gq - gk, -bnd), bnd) + bnd; }

// ------------------------------------------------------------------------------------ forward
// attn_fwd_kernel<0, NORM> of attention.hip (S^T = K Q^T: a lane owns one query, its accumulator registers run over the keys)
// with the position term added to the scaled scores.
template <bool NORM>
__global__ __launch_bounds__(256, 2) void attn_rpe_fwd_kernel(RpeP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  RpeSmem s = rpe_carve(smem, false);
  const int tid = threadIdx.x, wave = tid >> 6, l31 = tid & 31, hh = (tid >> 5) & 1;
  const int h = blockIdx.y, d = p.d, num = 2 * p.bnd + 1;
  const int q_start = p.tiles[blockIdx.x * 4 + 0], q_len = p.tiles[blockIdx.x * 4 + 1];
  const int k_start = p.tiles[blockIdx.x * 4 + 2], k_len = p.tiles[blockIdx.x * 4 + 3];

  if (tid < RT) {
    const int qr = tid < q_len ? (p.qidx ? p.qidx[q_start + tid] : q_start + tid) : -1;
    const int kr = tid < k_len ? (p.kidx ? p.kidx[k_start + tid] : k_start + tid) : -1;
    s.qrow[tid] = qr;
    s.krow[tid] = kr;
    s.qown[tid] = tid < q_len ? (p.owner ? p.owner[q_start + tid] : 1) : 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s.qg[3 * tid + a] = qr >= 0 ? p.grid[3L * qr + a] : 0;
      s.kg[3 * tid + a] = kr >= 0 ? p.grid[3L * kr + a] : 0;
    }
  } else if (tid - RT < 3 * num) {
    s.tab[tid - RT] = p.table[(long)(tid - RT) * p.H + h];
  }
  if constexpr (NORM) rpe_load_affine(p, s);
  __syncthreads();
  {
    const RpeRowSrc src[3] = {{s.Q, p.q, p.q_ld, p.q_off + h * d, s.qrow, q_len}, {s.K, p.kv, p.kv_ld, p.k_off + h * d, s.krow, k_len},
                              {s.V, p.kv, p.kv_ld, p.v_off + h * d, s.krow, k_len}};
    rpe_load_rows<3>(src, d);
  }
  __syncthreads();
  if constexpr (NORM) {
    if (tid < RT) rpe_ln_rows<true>(s.Q, s.qrstd, tid, q_len, d, p.eps, s.gq, s.bq);
    else rpe_ln_rows<true>(s.K, s.krstd, tid - RT, k_len, d, p.eps, s.gk, s.bk);
    __syncthreads();
  }

  const int r0 = wave * 32;
  if (r0 >= q_len) return;
  const int ktiles = (k_len + 31) / 32;
  const int qi = r0 + l31;  // this lane's query
  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = rpe_zero16();
  for (int kk = 0; kk < d; kk += 2) {
    const float bq = s.Q[qi * RLD + kk + hh];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (t < ktiles) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(s.K[(t * 32 + l31) * RLD + kk + hh], bq, acc[t], 0, 0, 0);
  }
  // scale, then the position term: three lookups in the head's table column per score
  const int g0 = s.qg[3 * qi], g1 = s.qg[3 * qi + 1], g2 = s.qg[3 * qi + 2];
  const float* tab0 = s.tab;
  const float* tab1 = s.tab + num;
  const float* tab2 = s.tab + 2 * num;
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
      float v = -INFINITY;
      if (key < k_len) {
        const int* kg = s.kg + 3 * key;
        const float bias = tab0[rpe_bin(g0, kg[0], p.bnd)] + tab1[rpe_bin(g1, kg[1], p.bnd)] + tab2[rpe_bin(g2, kg[2], p.bnd)];
        v = acc[t][r] * p.scale + bias;
      }
      acc[t][r] = v;
      m = fmaxf(m, v);
    }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float e = acc[t][r] > -INFINITY ? __expf(acc[t][r] - m) : 0.f;
      acc[t][r] = e;
      sum += e;
    }
  sum += __shfl_xor(sum, 32, 64);
  const float inv = sum > 0.f ? 1.f / sum : 0.f;
  if (p.drop_thresh) {
    const unsigned long long rb = (((unsigned long long)blockIdx.x * p.H + h) * RT + qi) * RT;
    const unsigned lo0 = (unsigned)rb, c2 = (unsigned)(rb >> 32) * 0x7FEB352Du + (unsigned)(p.drop_seed >> 32);
    const unsigned s0 = (unsigned)p.drop_seed;
    const float keep = inv * p.drop_inv_keep;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        acc[t][r] *= rpe_keep_lo(lo0 + (unsigned)(t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh), s0, c2, p.drop_thresh) ? keep : 0.f;
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] *= inv;
  }
  if (hh == 0 && qi < q_len && p.lse) p.lse[(long)(q_start + qi) * p.H + h] = m + logf(sum);
  // O^T[dcol][query] = sum_key V[key][dcol] P[query][key]
  f32x16 o = rpe_zero16();
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (t < ktiles) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        o = __builtin_amdgcn_mfma_f32_32x32x2f32(s.V[key * RLD + l31], acc[t][r], o, 0, 0, 0);
      }
    }
  if (qi < q_len && s.qown[qi]) {
    float* orow = p.out + (long)s.qrow[qi] * p.out_ld + h * d;
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int dc = 8 * q4 + 4 * hh;
      if (dc < d) st4(orow + dc, make_float4(o[4 * q4], o[4 * q4 + 1], o[4 * q4 + 2], o[4 * q4 + 3]));
    }
  }
}

// ------------------------------------------------------------------------------------ backward
// attn_bwd2_kernel<NORM> of attention.hip (S, P and dS exist once, lane <-> key; dQ through the LDS exchange image X aliased onto
// the V image) with the position term on the recomputed scores and the per-key bins of the table gradient.
typedef float rpe_f32x4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int rpe_xswz(int key) { return ((key & 1) << 2) | ((key >> 1) & 3); }

template <bool NORM>
__global__ __launch_bounds__(256, 1) void attn_rpe_bwd_kernel(RpeP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  RpeSmem s = rpe_carve(smem, true);
  __shared__ float lnacc[NORM ? 4 : 1][32];
  __shared__ float colred[NORM ? 2 : 1][NORM ? 8 : 1][32];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = tid & 31, hh = (tid >> 5) & 1;
  const int h = blockIdx.y, d = p.d, bnd = p.bnd, num = 2 * bnd + 1, nb = 3 * num;
  const int* bd = p.blocks + blockIdx.x * 6;
  const int first_tile = bd[0], n_tiles = bd[1], tile_step = bd[2], part_slot = bd[3];
  const int k_start = bd[4], k_len = bd[5];
  const int r0 = wave * 32;
  const int ktiles = (k_len + 31) / 32;
  float* X = s.V;  // dS exchange image [128 keys][32 queries], valid between the hoist of V and the dV staging

  if (tid < RT) {
    s.krow[tid] = tid < k_len ? (p.kidx ? p.kidx[k_start + tid] : k_start + tid) : -1;
    s.kext[tid] = (tid < k_len && p.kext) ? p.kext[k_start + tid] : -1;
  } else if (tid - RT < nb) {
    s.tab[tid - RT] = p.table[(long)(tid - RT) * p.H + h] * RPE_LOG2E;  // log2 units, as the recomputed scores
  }
  for (int i = tid; i < RT * nb; i += 256) s.bins[i] = 0.f;
  if constexpr (NORM) {
    if (tid < 4 * 32) lnacc[tid >> 5][tid & 31] = 0.f;
    rpe_load_affine(p, s);
  }
  __syncthreads();
  {
    const RpeRowSrc src[2] = {{s.K, p.kv, p.kv_ld, p.k_off + h * d, s.krow, k_len}, {s.V, p.kv, p.kv_ld, p.v_off + h * d, s.krow, k_len}};
    rpe_load_rows<2>(src, d);
  }
  __syncthreads();
  if constexpr (NORM) {
    if (tid >= RT) rpe_ln_rows<false>(s.K, s.krstd, tid - RT, k_len, d, p.eps, nullptr, nullptr);
    __syncthreads();
  }

  const float gq_l = NORM ? s.gq[l31] : 1.f, bq_l = NORM ? s.bq[l31] : 0.f;
  const float sl2 = p.scale * RPE_LOG2E;
  const bool has_keys = r0 < k_len;
  const int kj = r0 + l31;  // this lane's key
  const bool key_in = kj < k_len;
  float kb[16], vb[16], c_a = 0.f;
  int kg0 = 0, kg1 = 0, kg2 = 0;
  if (has_keys) {
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) {
      const int k = 2 * s2 + hh;
      if constexpr (NORM) {
        const float kn = s.K[kj * RLD + k] * s.gk[k] + s.bk[k];
        c_a += s.bq[k] * kn;
        kb[s2] = kn * s.gq[k] * sl2;
      } else {
        kb[s2] = s.K[kj * RLD + k] * sl2;
      }
      vb[s2] = s.V[kj * RLD + k];
    }
    if constexpr (NORM) {
      c_a += __shfl_xor(c_a, 32, 64);
      c_a = key_in ? c_a * sl2 : -INFINITY;
    } else {
      c_a = key_in ? 0.f : -INFINITY;
    }
    if (key_in) {
      const int* g = p.grid + 3L * s.krow[kj];
      kg0 = g[0]; kg1 = g[1]; kg2 = g[2];
    }
  }
  const float* tab0 = s.tab;
  const float* tab1 = s.tab + num;
  const float* tab2 = s.tab + 2 * num;
  float* mybins = s.bins + kj * nb;
  f32x16 acc_dv = rpe_zero16(), acc_dk = rpe_zero16();
  const int dh = wave & 1, qh = wave >> 1, l15 = lane & 15, kq = lane >> 4;
  const float gk_c = NORM ? s.gk[16 * dh + l15] : 1.f, bk_c = NORM ? s.bk[16 * dh + l15] : 0.f;
  __syncthreads();  // every wave holds its V fragment: the V image may become X

  for (int ti = 0; ti < n_tiles; ++ti) {
    const int tile = first_tile + ti * tile_step;
    const int q_start = p.tiles[tile * 4 + 0], q_len = p.tiles[tile * 4 + 1];
    if (tid < RT) {
      const int qr = tid < q_len ? (p.qidx ? p.qidx[q_start + tid] : q_start + tid) : -1;
      s.qrow[tid] = qr;
      s.qown[tid] = tid < q_len ? (p.owner ? p.owner[q_start + tid] : 1) : 0;
      s.lse[tid] = tid < q_len ? p.lse[(long)(q_start + tid) * p.H + h] * RPE_LOG2E : INFINITY;  // log2 units
#pragma unroll
      for (int a = 0; a < 3; ++a) s.qg[3 * tid + a] = qr >= 0 ? p.grid[3L * qr + a] : 0;
    }
    __syncthreads();
    {  // Q rows, dO rows (zero for non-owners) and D = rowsum(dO * O)
      const int sub = tid & 7, rr0 = tid >> 3;
      float4 qv[4], gv[4], ov[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = rr0 + 32 * j;
        qv[j] = gv[j] = ov[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < q_len && sub * 4 < d) {
          qv[j] = ld4(p.q + (long)s.qrow[r] * p.q_ld + p.q_off + h * d + sub * 4);
          if (s.qown[r]) {
            const long o = (long)s.qrow[r] * p.out_ld + h * d + sub * 4;
            gv[j] = ld4(p.dout + o);
            ov[j] = ld4(p.out + o);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = rr0 + 32 * j;
        float* oq = s.Q + r * RLD + sub * 4;
        oq[0] = qv[j].x; oq[1] = qv[j].y; oq[2] = qv[j].z; oq[3] = qv[j].w;
        float* o = s.dO + r * RLD + sub * 4;
        o[0] = gv[j].x; o[1] = gv[j].y; o[2] = gv[j].z; o[3] = gv[j].w;
        float dsum = gv[j].x * ov[j].x + gv[j].y * ov[j].y + gv[j].z * ov[j].z + gv[j].w * ov[j].w;
        dsum += __shfl_xor(dsum, 1, 64);
        dsum += __shfl_xor(dsum, 2, 64);
        dsum += __shfl_xor(dsum, 4, 64);
        if (sub == 0) s.Dv[r] = dsum;
      }
    }
    __syncthreads();
    if constexpr (NORM) {
      if (tid < RT) rpe_ln_rows<false>(s.Q, s.qrstd, tid, q_len, d, p.eps, nullptr, nullptr);
      __syncthreads();
    }

    const unsigned long long tb = ((unsigned long long)tile * p.H + h) * RT * RT;
    const unsigned c2 = (unsigned)(tb >> 32) * 0x7FEB352Du + (unsigned)(p.drop_seed >> 32);
    const unsigned x_lane = ((unsigned)tb + (unsigned)kj + (unsigned)(4 * hh * RT)) * 0x9E3779B1u + (unsigned)p.drop_seed;
    const int qtiles = (q_len + 31) / 32;
    for (int qt = 0; qt < qtiles; ++qt) {
      f32x16 sa, dpa;
      if (has_keys) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { sa[r] = c_a; dpa[r] = 0.f; }
        const float* qrow_p = s.Q + (qt * 32 + l31) * RLD + hh;
        const float* dorow_p = s.dO + (qt * 32 + l31) * RLD + hh;
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) {
          sa = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow_p[2 * s2], kb[s2], sa, 0, 0, 0);
          dpa = __builtin_amdgcn_mfma_f32_32x32x2f32(dorow_p[2 * s2], vb[s2], dpa, 0, 0, 0);
        }
        float lse4[16], d4[16];
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const float4 a = ld4(s.lse + qt * 32 + 8 * q4 + 4 * hh);
          const float4 b = ld4(s.Dv + qt * 32 + 8 * q4 + 4 * hh);
          lse4[4 * q4] = a.x; lse4[4 * q4 + 1] = a.y; lse4[4 * q4 + 2] = a.z; lse4[4 * q4 + 3] = a.w;
          d4[4 * q4] = b.x; d4[4 * q4 + 1] = b.y; d4[4 * q4 + 2] = b.z; d4[4 * q4 + 3] = b.w;
        }
        const unsigned xq = x_lane + (unsigned)(qt * 32 * RT) * 0x9E3779B1u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int qq = qt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
          const int* qg = s.qg + 3 * qq;
          const int i0 = rpe_bin(qg[0], kg0, bnd), i1 = rpe_bin(qg[1], kg1, bnd), i2 = rpe_bin(qg[2], kg2, bnd);
          const float e = __builtin_amdgcn_exp2f(sa[r] + (tab0[i0] + tab1[i1] + tab2[i2]) - lse4[r]);
          float t = 1.f;
          if (p.drop_thresh) {
            unsigned x = xq + (unsigned)(((r & 3) + 8 * (r >> 2)) * RT) * 0x9E3779B1u;
            x ^= c2;
            x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15;
            t = x >= p.drop_thresh ? p.drop_inv_keep : 0.f;
          }
          sa[r] = e * t;                          // dropout(P)
          const float g = e * (dpa[r] * t - d4[r]);  // gradient of the pre-softmax score: what the table receives
          dpa[r] = g * p.scale;                   // dS
          // the table gradient: the lower lane half adds its own value, then its partner's (same key, query qq + 4)
          const float gp = __shfl_xor(g, 32, 64);
          if (hh == 0 && key_in) {
            if (qq < q_len) {
              mybins[i0] += g;
              mybins[num + i1] += g;
              mybins[2 * num + i2] += g;
            }
            if (qq + 4 < q_len) {
              const int* qp = qg + 12;
              mybins[rpe_bin(qp[0], kg0, bnd)] += gp;
              mybins[num + rpe_bin(qp[1], kg1, bnd)] += gp;
              mybins[2 * num + rpe_bin(qp[2], kg2, bnd)] += gp;
            }
          }
        }
      }
      __syncthreads();  // (A) the dQ products of the previous query tile are done with X
      if (has_keys) {
        float* xr = X + kj * 32;
        const int sw = rpe_xswz(kj);
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<float4*>(xr + (((2 * g + hh) ^ sw) << 2)) = make_float4(dpa[4 * g], dpa[4 * g + 1], dpa[4 * g + 2], dpa[4 * g + 3]);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int qq = qt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
          acc_dv = __builtin_amdgcn_mfma_f32_32x32x2f32(s.dO[qq * RLD + l31], sa[r], acc_dv, 0, 0, 0);
          if constexpr (NORM) acc_dk = __builtin_amdgcn_mfma_f32_32x32x2f32(s.Q[qq * RLD + l31] * gq_l + bq_l, dpa[r], acc_dk, 0, 0, 0);
          else acc_dk = __builtin_amdgcn_mfma_f32_32x32x2f32(s.Q[qq * RLD + l31], dpa[r], acc_dk, 0, 0, 0);
        }
      }
      __syncthreads();  // (B) X holds dS of every key for this query tile
      {
        rpe_f32x4v acc = {0.f, 0.f, 0.f, 0.f};
        const int ql = 16 * qh + l15;
        const float* kcol = s.K + 16 * dh + l15;
        for (int t = 0; t < ktiles; ++t) {
#pragma unroll
          for (int s4 = 0; s4 < 8; ++s4) {
            const int key = 32 * t + 4 * s4 + kq;
            const float a = NORM ? kcol[key * RLD] * gk_c + bk_c : kcol[key * RLD];
            const float b = X[key * 32 + ((((ql >> 2) ^ rpe_xswz(key)) << 2) | (ql & 3))];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
          }
        }
        float* o = s.dO + (qt * 32 + ql) * RLD + 16 * dh + 4 * kq;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = acc[3];
      }
    }
    __syncthreads();
    if constexpr (NORM) {
      const int j = tid & 31, part = tid >> 5;
      float ag = 0.f, ab = 0.f;
      if (j < d)
        for (int r = part * 16; r < min(q_len, part * 16 + 16); ++r) {
          const float g = s.dO[r * RLD + j];
          ag += g * s.Q[r * RLD + j];
          ab += g;
        }
      colred[0][part][j] = ag;
      colred[1][part][j] = ab;
      __syncthreads();
      if (tid < 64) {
        const int which = tid >> 5, j2 = tid & 31;  // 0: dgamma_q, 1: dbeta_q
        float a = 0.f;
        for (int k = 0; k < 8; ++k) a += colred[which][k][j2];
        lnacc[which][j2] += a;
      }
      if (tid < RT) rpe_ln_rows_bwd(s.dO, s.Q, s.qrstd, tid, q_len, d, s.gq);
      __syncthreads();
    }
    rpe_store_rows(s.dO, p.dq, p.dq_ld, p.dq_off + h * d, s.qrow, s.qown, q_len, d);
    __syncthreads();
  }

  // ---- the table gradient of this (block, head): the keys' bins in ascending key order, in float64
  if (tid < nb) {
    double a = 0.0;
    for (int k = 0; k < k_len; ++k) a += (double)s.bins[k * nb + tid];
    p.tab_part[((long)blockIdx.x * p.H + h) * nb + tid] = a;
  }
  // ---- K / V gradients of this block
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int dc = (r & 3) + 8 * (r >> 2) + 4 * hh;
    s.V[(r0 + l31) * RLD + dc] = (dc < d) ? acc_dv[r] : 0.f;
    s.dO[(r0 + l31) * RLD + dc] = (dc < d) ? acc_dk[r] : 0.f;
  }
  __syncthreads();
  if constexpr (NORM) {
    const int j = tid & 31, part = tid >> 5;
    float ag = 0.f, ab = 0.f;
    if (j < d)
      for (int r = part * 16; r < min(k_len, part * 16 + 16); ++r) {
        const float g = s.dO[r * RLD + j];
        ag += g * s.K[r * RLD + j];
        ab += g;
      }
    colred[0][part][j] = ag;
    colred[1][part][j] = ab;
    __syncthreads();
    if (tid < 64) {
      const int which = tid >> 5, j2 = tid & 31;  // 2: dgamma_k, 3: dbeta_k
      float a = 0.f;
      for (int k = 0; k < 8; ++k) a += colred[which][k][j2];
      lnacc[2 + which][j2] = a;
    }
    if (tid < RT) rpe_ln_rows_bwd(s.dO, s.K, s.krstd, tid, k_len, d, s.gk);
    __syncthreads();
  }
  float* dkv = p.dkv + (long)part_slot * p.dkv_part_stride;
  rpe_store_rows(s.dO, dkv, p.dkv_ld, p.dk_off + h * d, s.krow, nullptr, k_len, d, p.dkv_extra ? s.kext : nullptr, p.dkv_extra,
                 p.dkv_extra_ld, h * d);
  rpe_store_rows(s.V, dkv, p.dkv_ld, p.dv_off + h * d, s.krow, nullptr, k_len, d, p.dkv_extra ? s.kext : nullptr, p.dkv_extra,
                 p.dkv_extra_ld, p.dv_off - p.dk_off + h * d);
  if constexpr (NORM)
    if (tid < 128) p.ln_part[((long)(blockIdx.x * p.H + h) * 4 + (tid >> 5)) * 32 + (tid & 31)] = lnacc[tid >> 5][tid & 31];
}

// dtable[r][h] = sum over the blocks, ascending, of part[block][h][r] in float64 (written; nblocks == 0 writes zeros)
__global__ __launch_bounds__(256) void attn_rpe_merge_kernel(const double* __restrict__ part, float* __restrict__ dtable, int nblocks,
                                                             int H, int nb) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nb * H) return;
  const int r = e / H, h = e - r * H;
  double sum = 0.0;
  for (int b = 0; b < nblocks; ++b) sum += part[((long)b * H + h) * nb + r];
  dtable[e] = (float)sum;
}

// out[which][j] (+)= sum_b part[b][which][j]: fixed-order tree (attn_ln_reduce_kernel of attention.hip)
__global__ __launch_bounds__(1024) void attn_rpe_ln_reduce_kernel(const float* __restrict__ part, float* o0, float* o1, float* o2,
                                                                  float* o3, int nb, int d, int accumulate) {
  __shared__ float red[32][33];
  const int which = blockIdx.x, j = threadIdx.x & 31, r = threadIdx.x >> 5;
  float s = 0.f;
  int b = r;
  for (; b + 96 < nb; b += 128) {
    const float v0 = part[((long)b * 4 + which) * 32 + j], v1 = part[((long)(b + 32) * 4 + which) * 32 + j];
    const float v2 = part[((long)(b + 64) * 4 + which) * 32 + j], v3 = part[((long)(b + 96) * 4 + which) * 32 + j];
    s += (v0 + v1) + (v2 + v3);
  }
  for (; b < nb; b += 32) s += part[((long)b * 4 + which) * 32 + j];
  red[r][j] = s;
  __syncthreads();
  if (r == 0 && j < d) {
    float t = 0.f;
    for (int k = 0; k < 32; ++k) t += red[k][j];
    float* o = which == 0 ? o0 : which == 1 ? o1 : which == 2 ? o2 : o3;
    o[j] = accumulate ? o[j] + t : t;
  }
}

// dqkv[point][k|v columns] += extra[e] for every borrowed copy e (each point is borrowed at most once)
__global__ void attn_rpe_extra_fixup_kernel(const float* __restrict__ extra, long extra_ld, const int* __restrict__ ext_pos,
                                            const int* __restrict__ kidx, int n_extra, int w4, float* __restrict__ dkv, long dkv_ld,
                                            int dk_off) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)n_extra * w4) return;
  const int e = (int)(gid / w4), c = (int)(gid % w4) * 4;
  const int point = kidx[ext_pos[e]];
  const float4 a = ld4(extra + (long)e * extra_ld + c);
  float* o = dkv + (long)point * dkv_ld + dk_off + c;
  float4 v = ld4(o);
  v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
  st4(o, v);
}

static void rpe_set_drop(RpeP& p, float drop_p, unsigned long long seed) {
  p.drop_seed = seed;
  p.drop_thresh = 0;
  p.drop_inv_keep = 1.f;
  if (drop_p > 0.f) {
    p.drop_thresh = (unsigned)(drop_p * 4294967296.0);
    if (p.drop_thresh == 0) p.drop_thresh = 1;
    p.drop_inv_keep = 1.f / (1.f - drop_p);
  }
}

static int rpe_norm_mode(const float* qn_w, const float* qn_b, const float* kn_w, const float* kn_b) {
  const int n = (qn_w != nullptr) + (qn_b != nullptr) + (kn_w != nullptr) + (kn_b != nullptr);
  return n == 4 ? 1 : n == 0 ? 0 : -1;
}

// what both entry points refuse alike
static int rpe_check(const char* who, int H, int d, const int* grid, const float* table, int bnd, float drop_p) {
  LOTUS_CHECK_ARG(H > 0 && d >= 4 && d <= 32 && d % 4 == 0, "%s: H = %d, d = %d (H > 0; d a multiple of 4 up to 32)", who, H, d);
  LOTUS_CHECK_ARG(bnd >= 0, "%s: bnd = %d must not be negative", who, bnd);
  LOTUS_CHECK_ARG(bnd <= RPE_MAX_BND, "%s: bnd = %d > %d (the pos_bnd of a 128-row patch; the head's table column is held in LDS)",
                  who, bnd, RPE_MAX_BND);
  LOTUS_CHECK_ARG(!(table && !grid), "%s: a table without grid coordinates (grid is null)", who);
  LOTUS_CHECK_ARG(table && grid, "%s: null pointer (table, grid)", who);
  LOTUS_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "%s: drop_p = %g outside [0, 1)", who, (double)drop_p);
  return LOTUS_OK;
}

extern "C" {

int lotus_attention_rpe_fwd(const float* q, long q_ld, int q_off, const float* kv, long kv_ld, int k_off, int v_off, const int* qidx,
                            const int* kidx, const int* owner, const int* tiles, int ntiles, const float* qn_w, const float* qn_b,
                            const float* kn_w, const float* kn_b, float* out, long out_ld, float* lse, int H, int d, float scale,
                            float eps, float drop_p, unsigned long long drop_seed, const int* grid, const float* table, int bnd,
                            void* stream) {
  LOTUS_CHECK_ARG(q && kv && tiles && out, "lotus_attention_rpe_fwd: null pointer (q, kv, tiles, out)");
  const int rc = rpe_check("lotus_attention_rpe_fwd", H, d, grid, table, bnd, drop_p);
  if (rc) return rc;
  const int norm = rpe_norm_mode(qn_w, qn_b, kn_w, kn_b);
  LOTUS_CHECK_ARG(norm >= 0, "lotus_attention_rpe_fwd: qn_w, qn_b, kn_w, kn_b must be all given or all null");
  LOTUS_CHECK_ARG(ntiles >= 0, "lotus_attention_rpe_fwd: ntiles = %d must not be negative", ntiles);
  if (ntiles == 0) return LOTUS_OK;
  RpeP p;
  memset(&p, 0, sizeof(p));
  p.q = q; p.q_ld = q_ld; p.q_off = q_off; p.kv = kv; p.kv_ld = kv_ld; p.k_off = k_off; p.v_off = v_off;
  p.qidx = qidx; p.kidx = kidx; p.owner = owner; p.tiles = tiles;
  p.qn_w = qn_w; p.qn_b = qn_b; p.kn_w = kn_w; p.kn_b = kn_b;
  p.out = out; p.out_ld = out_ld; p.lse = lse; p.H = H; p.d = d; p.scale = scale; p.eps = eps;
  p.grid = grid; p.table = table; p.bnd = bnd;
  rpe_set_drop(p, drop_p, drop_seed);
  const size_t lds = rpe_smem_bytes(false, bnd);
  lotus_note_attn_route(LOTUS_ATTN_RPE_FWD, 0, 0, 0, norm, 256, (int)lds, 0);
  const dim3 g(ntiles, H), b(256);
  if (norm) {
    lotus_allow_dyn_lds_once<attn_rpe_fwd_kernel<true>>(rpe_smem_bytes(false, RPE_MAX_BND));
    LOTUS_LAUNCH(attn_rpe_fwd_kernel<true>, g, b, lds, (hipStream_t)stream, p);
  } else {
    lotus_allow_dyn_lds_once<attn_rpe_fwd_kernel<false>>(rpe_smem_bytes(false, RPE_MAX_BND));
    LOTUS_LAUNCH(attn_rpe_fwd_kernel<false>, g, b, lds, (hipStream_t)stream, p);
  }
  LOTUS_LAUNCH_CHECK("lotus_attention_rpe_fwd");
  return LOTUS_OK;
}

size_t lotus_attention_rpe_bwd_workspace(int nblocks, int H, int bnd) {
  if (nblocks < 0 || H <= 0 || bnd < 0) return 0;
  const size_t bh = (size_t)nblocks * H;
  return bh * 4 * 32 * sizeof(float) + bh * 3 * (2 * (size_t)bnd + 1) * sizeof(double);
}

int lotus_attention_rpe_bwd(const float* q, long q_ld, int q_off, const float* kv, long kv_ld, int k_off, int v_off, const int* qidx,
                            const int* kidx, const int* owner, const int* tiles, const int* blocks, int nblocks, const float* qn_w,
                            const float* qn_b, const float* kn_w, const float* kn_b, const float* out, const float* dout, long out_ld,
                            const float* lse, float* dq, long dq_ld, int dq_off, float* dkv, long dkv_ld, int dk_off, int dv_off,
                            long dkv_part_stride, const int* kext, const int* ext_pos, int n_extra, float* dkv_extra, float* dqn_w,
                            float* dqn_b, float* dkn_w, float* dkn_b, int accumulate, int H, int d, float scale, float eps, float drop_p,
                            unsigned long long drop_seed, const int* grid, const float* table, int bnd, float* dtable, void* workspace,
                            size_t workspace_bytes, void* stream) {
  LOTUS_CHECK_ARG(q && kv && tiles && blocks && out && dout && lse && dq && dkv && dtable,
                  "lotus_attention_rpe_bwd: null pointer (q, kv, tiles, blocks, out, dout, lse, dq, dkv, dtable)");
  const int rc = rpe_check("lotus_attention_rpe_bwd", H, d, grid, table, bnd, drop_p);
  if (rc) return rc;
  const int norm = rpe_norm_mode(qn_w, qn_b, kn_w, kn_b);
  LOTUS_CHECK_ARG(norm >= 0, "lotus_attention_rpe_bwd: qn_w, qn_b, kn_w, kn_b must be all given or all null");
  LOTUS_CHECK_ARG(!norm || (dqn_w && dqn_b && dkn_w && dkn_b), "lotus_attention_rpe_bwd: null norm gradient");
  LOTUS_CHECK_ARG(nblocks >= 0, "lotus_attention_rpe_bwd: nblocks = %d must not be negative", nblocks);
  LOTUS_CHECK_ARG(nblocks == 0 || (workspace && ((uintptr_t)workspace) % 8 == 0 &&
                                   workspace_bytes >= lotus_attention_rpe_bwd_workspace(nblocks, H, bnd)),
                  "lotus_attention_rpe_bwd: workspace too small or misaligned (lotus_attention_rpe_bwd_workspace(nblocks, H, bnd) bytes)");
  const bool extra = kext && n_extra > 0;
  LOTUS_CHECK_ARG(!extra || (dkv_extra && ext_pos && kidx && dv_off - dk_off == H * d),
                  "lotus_attention_rpe_bwd: borrowed-row buffer needs dkv_extra, ext_pos, kidx and adjacent k|v column blocks");
  hipStream_t st = (hipStream_t)stream;
  const int nb = 3 * (2 * bnd + 1);
  StopEventOnLast stop_ev;
  if (nblocks == 0) {  // nothing to walk: the table gradient is still written (zeros); the route record stays
    stop_ev.last();
    LOTUS_LAUNCH(attn_rpe_merge_kernel, dim3(cdiv((long)nb * H, 256)), dim3(256), 0, st, (const double*)nullptr, dtable, 0, H, nb);
    LOTUS_LAUNCH_CHECK("lotus_attention_rpe_bwd");
    return LOTUS_OK;
  }
  RpeP p;
  memset(&p, 0, sizeof(p));
  p.q = q; p.q_ld = q_ld; p.q_off = q_off; p.kv = kv; p.kv_ld = kv_ld; p.k_off = k_off; p.v_off = v_off;
  p.qidx = qidx; p.kidx = kidx; p.owner = owner; p.tiles = tiles; p.blocks = blocks;
  p.qn_w = qn_w; p.qn_b = qn_b; p.kn_w = kn_w; p.kn_b = kn_b;
  p.out = (float*)out; p.dout = dout; p.out_ld = out_ld; p.lse = (float*)lse;
  p.dq = dq; p.dq_ld = dq_ld; p.dq_off = dq_off;
  p.dkv = dkv; p.dkv_ld = dkv_ld; p.dk_off = dk_off; p.dv_off = dv_off; p.dkv_part_stride = dkv_part_stride;
  p.ln_part = (float*)workspace;
  p.tab_part = (double*)((float*)workspace + (size_t)nblocks * H * 4 * 32);
  p.kext = kext; p.dkv_extra = extra ? dkv_extra : nullptr; p.dkv_extra_ld = 2L * H * d;
  p.grid = grid; p.table = table; p.bnd = bnd;
  p.H = H; p.d = d; p.scale = scale; p.eps = eps;
  rpe_set_drop(p, drop_p, drop_seed);
  const size_t lds = rpe_smem_bytes(true, bnd);
  const int tail = (extra ? LOTUS_ATTN_TAIL_FIXUP : 0) | (norm ? LOTUS_ATTN_TAIL_LN_REDUCE : 0) | LOTUS_ATTN_TAIL_RPE_MERGE;
  lotus_note_attn_route(LOTUS_ATTN_RPE_BWD, 1, 0, 0, norm, 256, (int)lds, tail);
  const dim3 g(nblocks, H), b(256);
  if (norm) {
    lotus_allow_dyn_lds_once<attn_rpe_bwd_kernel<true>>(rpe_smem_bytes(true, RPE_MAX_BND));
    LOTUS_LAUNCH(attn_rpe_bwd_kernel<true>, g, b, lds, st, p);
  } else {
    lotus_allow_dyn_lds_once<attn_rpe_bwd_kernel<false>>(rpe_smem_bytes(true, RPE_MAX_BND));
    LOTUS_LAUNCH(attn_rpe_bwd_kernel<false>, g, b, lds, st, p);
  }
  if (extra) {
    const int w4 = 2 * H * d / 4;
    LOTUS_LAUNCH(attn_rpe_extra_fixup_kernel, dim3(cdiv((long)n_extra * w4, 256)), dim3(256), 0, st, (const float*)dkv_extra,
                 2L * H * d, ext_pos, kidx, n_extra, w4, dkv, dkv_ld, dk_off);
  }
  if (norm)
    LOTUS_LAUNCH(attn_rpe_ln_reduce_kernel, dim3(4), dim3(1024), 0, st, (const float*)p.ln_part, dqn_w, dqn_b, dkn_w, dkn_b,
                 nblocks * H, d, accumulate);
  stop_ev.last();
  LOTUS_LAUNCH(attn_rpe_merge_kernel, dim3(cdiv((long)nb * H, 256)), dim3(256), 0, st, (const double*)p.tab_part, dtable, nblocks,
               H, nb);
  LOTUS_LAUNCH_CHECK("lotus_attention_rpe_bwd");
  return LOTUS_OK;
}

}  // extern "C"

}  // namespace LOTUS_NS
