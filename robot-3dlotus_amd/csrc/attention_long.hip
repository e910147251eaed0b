// lotus-hip: patch attention for patches above 128 rows (PointTransformerV3/model.py:529-551: SerializedAttention over patches of
// enc_patch_size / dec_patch_size = 256, 512, 1024 points).  The tile kernels of attention.hip and attention_rpe.hip hold ONE
// 128-row key image in LDS; here a tile may have q_len, k_len up to LOTUS_ATTN_LONG_MAX = 1024 and the keys are walked in 128-row
// images, all in exact fp32 (v_mfma_f32_32x32x2_f32).  Those files are not touched; what is needed of them — the per-row
// LayerNorm, the dropout hash, the fix-up of borrowed rows — is restated here.
//   forward   one block per (128-row query slab of a tile, head).  S^T = K Q^T, 32 keys of the image at a time: a lane owns one
//             query, its 16 accumulator registers run over the keys.  Online softmax: the running maximum m and sum l of the
//             lane's query; when keys raise m the output accumulator and l are rescaled by exp(m_old - m_new).  The output is
//             divided by l at the end; lse = m + log l, one per (row, head).
//   backward  delta = rowsum(dO o O) is computed once, by the dQ kernel (which loads both anyway), into the workspace.
//             dQ     one block per (query slab, head) walks the key images: S^T and dP^T per 32 keys, dS^T in registers,
//                    dQ^T += K^T dS^T (the lane owns the query, as in the forward).
//             dK/dV  one block per (key image, head) walks the query slabs: a lane owns one key (attn_bwd2_kernel's layout without
//                    its dQ exchange); the block owns its 128 output rows and writes them with plain stores, borrowed rows into
//                    dkv_extra (kext / ext_pos protocol).
//             The q/k-norm parameter gradients are summed per block in fp32, then over the blocks in ascending order in float64.
//             No atomics anywhere: reruns are bit-identical.
// The next key image's global loads are issued before the current image's products (forward and dQ); every lane loads with its
// row and column clamped into the valid range and selects afterwards, so no load of the key loop sits under a branch.
// Dropout element of (tile, head h, query i, key j), i and j counted from the tile's q_start / k_start:
//   idx = ((tile * H + h) * 1024 + i) * 1024 + j,  keep iff mix(seed, idx) >= thresh   (the mask function of attention.hip)
// fp32 storage only (no bf16 twin).
#include "mma.h"
#include "attn_route.h"

namespace LOTUS_NS {

#define LT 128        // rows of a query slab / a key image
#define LLD 33        // row stride of the [128][d <= 32] images
#define LNG_MAX 1024  // LOTUS_ATTN_LONG_MAX of include/lotus_hip.h
#define LNG_LOG2E 1.4426950408889634f

struct LngP {
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
  float* delta;    // [npos][H]  rowsum(dO o O), written by the dQ kernel, read by the dK/dV kernel
  float* ln_part;  // [nblocks * slabs * H][4][32]  dgamma_q, dbeta_q (dQ kernel), dgamma_k, dbeta_k (dK/dV kernel)
  const int* kext; float* dkv_extra; long dkv_extra_ld;
  int slabs;  // 128-row slabs per tile the grid provides: ceil(len_max / 128)
  int H, d;
  float scale, eps;
  unsigned long long drop_seed;
  unsigned drop_thresh;
  float drop_inv_keep;
};

// keep iff mix(seed, idx) >= thresh; lo = low word of idx, c2 = (high word of idx) * 0x7FEB352D + high word of the seed
__device__ __forceinline__ bool lng_keep_lo(unsigned lo, unsigned s0, unsigned c2, unsigned thresh) {
  unsigned x = lo * 0x9E3779B1u + s0;
  x ^= c2;
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15;
  return x >= thresh;
}

__device__ __forceinline__ f32x16 lng_zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

// One image of gathered rows in flight: 4 x 16 bytes per thread.  issue: every lane loads, row clamped to cnt - 1 (cnt >= 1) and
// column to d - 4; commit: rows >= cnt and columns >= d become zero.
struct LngStage { float4 v[4]; };
__device__ __forceinline__ void lng_issue(LngStage& st, const float* base, long ld, int coff, const int* rows_s, int cnt, int d) {
  const int sub = threadIdx.x & 7, r0 = threadIdx.x >> 3;
  const int c = min(sub * 4, d - 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = min(r0 + 32 * j, cnt - 1);
    st.v[j] = ld4(base + (long)rows_s[r] * ld + coff + c);
  }
}
__device__ __forceinline__ void lng_commit(const LngStage& st, float* img, int cnt, int d) {
  const int sub = threadIdx.x & 7, r0 = threadIdx.x >> 3;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = r0 + 32 * j;
    const bool ok = r < cnt && sub * 4 < d;
    float* o = img + r * LLD + sub * 4;
    o[0] = ok ? st.v[j].x : 0.f; o[1] = ok ? st.v[j].y : 0.f; o[2] = ok ? st.v[j].z : 0.f; o[3] = ok ? st.v[j].w : 0.f;
  }
}

template <bool AFFINE>
__device__ __forceinline__ void lng_ln_rows(float* img, float* rstd_s, int row, int len, int d, float eps, const float* g_s,
                                            const float* b_s) {
  if (row >= len) {
    if (row < LT) rstd_s[row] = 0.f;
    return;
  }
  float* x = img + row * LLD;
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

// g: gradient of the normalised, affine rows; xh: the normalised rows (no affine) -> g becomes the gradient of the raw rows
__device__ __forceinline__ void lng_ln_rows_bwd(float* g, const float* xh, const float* rstd_s, int row, int len, int d,
                                                const float* gam) {
  if (row >= len) return;
  float* gr = g + row * LLD;
  const float* xr = xh + row * LLD;
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
__device__ __forceinline__ void lng_store_rows(const float* img, float* base, long ld, int coff, const int* rows_s, const int* own_s,
                                               int len, int d, const int* ext_s = nullptr, float* ext_base = nullptr,
                                               long ext_ld = 0, int ext_coff = 0) {
  const int sub = threadIdx.x & 7;
  for (int r = threadIdx.x >> 3; r < len; r += 32) {
    if (own_s && !own_s[r]) continue;
    if (sub * 4 >= d) continue;
    const float* v = img + r * LLD + sub * 4;
    float* o = base + (long)rows_s[r] * ld + coff + sub * 4;
    if (ext_s && ext_s[r] >= 0) o = ext_base + (long)ext_s[r] * ext_ld + ext_coff + sub * 4;
    st4(o, make_float4(v[0], v[1], v[2], v[3]));
  }
}

// the LDS of the three kernels (floats unless noted): row images, per-row scalars, the norm's affine vectors, the slab's row
// tables and the row numbers of ALL keys of the tile (the next image's loads are issued from it)
struct LngSmem {
  float* Q; float* K; float* V; float* dO;
  float* qrstd; float* krstd; float* Dv; float* lse;
  float* gq; float* bq; float* gk; float* bk;
  int* qrow; int* qown; int* krow;  // krow[LNG_MAX]; the dK/dV kernel keeps krow[128] | kext[128] there
};
__device__ __forceinline__ LngSmem lng_carve(float* base, bool bwd) {
  LngSmem s;
  float* p = base;
  s.Q = p; p += LT * LLD;
  s.K = p; p += LT * LLD;
  s.V = p; p += LT * LLD;
  s.dO = p; if (bwd) p += LT * LLD;
  s.qrstd = p; p += LT;
  s.krstd = p; p += LT;
  s.Dv = p; if (bwd) p += LT;
  s.lse = p; if (bwd) p += LT;
  s.gq = p; p += 32; s.bq = p; p += 32; s.gk = p; p += 32; s.bk = p; p += 32;
  s.qrow = (int*)p; p += LT;
  s.qown = (int*)p; p += LT;
  s.krow = (int*)p;
  return s;
}
static size_t lng_smem_bytes(bool bwd) {
  return ((bwd ? 4 : 3) * LT * LLD + (bwd ? 4 : 2) * LT + 4 * 32 + 2 * LT + LNG_MAX) * sizeof(float);
}

__device__ __forceinline__ void lng_load_affine(const LngP& p, LngSmem& s) {
  const int t = threadIdx.x;
  if (t < 32) {
    const bool in = t < p.d;
    s.gq[t] = in ? p.qn_w[t] : 0.f;
    s.bq[t] = in ? p.qn_b[t] : 0.f;
    s.gk[t] = in ? p.kn_w[t] : 0.f;
    s.bk[t] = in ? p.kn_b[t] : 0.f;
  }
}

// ------------------------------------------------------------------------------------ forward
template <bool NORM>
__global__ __launch_bounds__(256, 2) void attn_long_fwd_kernel(LngP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  LngSmem s = lng_carve(smem, false);
  const int tid = threadIdx.x, wave = tid >> 6, l31 = tid & 31, hh = (tid >> 5) & 1;
  const int h = blockIdx.y, d = p.d;
  const int tile = blockIdx.x / p.slabs, q0 = (blockIdx.x % p.slabs) * LT;
  const int q_start = p.tiles[tile * 4 + 0], q_len = p.tiles[tile * 4 + 1];
  const int k_start = p.tiles[tile * 4 + 2], k_len = min(p.tiles[tile * 4 + 3], LNG_MAX);
  if (q0 >= q_len) return;
  const int qcnt = min(LT, q_len - q0);

  if (tid < LT) {
    s.qrow[tid] = tid < qcnt ? (p.qidx ? p.qidx[q_start + q0 + tid] : q_start + q0 + tid) : -1;
    s.qown[tid] = tid < qcnt ? (p.owner ? p.owner[q_start + q0 + tid] : 1) : 0;
  }
  for (int i = tid; i < k_len; i += 256) s.krow[i] = p.kidx ? p.kidx[k_start + i] : k_start + i;
  if constexpr (NORM) lng_load_affine(p, s);
  __syncthreads();
  const int qi = wave * 32 + l31;  // this lane's query of the slab
  if (k_len <= 0) {                // no keys: zero rows, lse = -inf
    if (qi < qcnt && hh == 0) {
      if (p.lse) p.lse[(long)(q_start + q0 + qi) * p.H + h] = -INFINITY;
      if (s.qown[qi])
        for (int c = 0; c < d; c += 4) st4(p.out + (long)s.qrow[qi] * p.out_ld + h * d + c, make_float4(0.f, 0.f, 0.f, 0.f));
    }
    return;
  }
  const int nimg = (k_len + LT - 1) / LT;
  LngStage sk, sv;
  {
    LngStage sq;
    lng_issue(sq, p.q, p.q_ld, p.q_off + h * d, s.qrow, qcnt, d);
    lng_issue(sk, p.kv, p.kv_ld, p.k_off + h * d, s.krow, min(LT, k_len), d);
    lng_issue(sv, p.kv, p.kv_ld, p.v_off + h * d, s.krow, min(LT, k_len), d);
    lng_commit(sq, s.Q, qcnt, d);
  }

  const bool active = wave * 32 < qcnt;
  float m_run = -INFINITY, l_run = 0.f;
  f32x16 o = lng_zero16();
  const unsigned long long rb = ((((unsigned long long)tile * p.H + h) * LNG_MAX) + (unsigned)(q0 + qi)) * LNG_MAX;
  const unsigned lo0 = (unsigned)rb, c2 = (unsigned)(rb >> 32) * 0x7FEB352Du + (unsigned)(p.drop_seed >> 32);
  const unsigned s0 = (unsigned)p.drop_seed;

  for (int j = 0; j < nimg; ++j) {
    const int kcnt = min(LT, k_len - j * LT);
    __syncthreads();  // the previous image's products are done with K and V
    lng_commit(sk, s.K, kcnt, d);
    lng_commit(sv, s.V, kcnt, d);
    __syncthreads();
    if constexpr (NORM) {
      if (tid < LT) {
        if (j == 0) lng_ln_rows<true>(s.Q, s.qrstd, tid, qcnt, d, p.eps, s.gq, s.bq);
      } else {
        lng_ln_rows<true>(s.K, s.krstd, tid - LT, kcnt, d, p.eps, s.gk, s.bk);
      }
      __syncthreads();
    }
    {  // the next image's rows (the last image once more at the end: no branch around a load)
      const int jn = min(j + 1, nimg - 1), ncnt = min(LT, k_len - jn * LT);
      lng_issue(sk, p.kv, p.kv_ld, p.k_off + h * d, s.krow + jn * LT, ncnt, d);
      lng_issue(sv, p.kv, p.kv_ld, p.v_off + h * d, s.krow + jn * LT, ncnt, d);
    }
    if (!active) continue;
    const int ktiles = (kcnt + 31) / 32;
    for (int t = 0; t < ktiles; ++t) {  // 32 keys at a time: scores, running maximum and sum, rescale, P V
      f32x16 acc = lng_zero16();
      const float* krow_p = s.K + (t * 32 + l31) * LLD + hh;
      const float* qrow_p = s.Q + qi * LLD + hh;
      for (int kk = 0; kk < d; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(krow_p[kk], qrow_p[kk], acc, 0, 0, 0);
      float mi = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        const float v = key < kcnt ? acc[r] * p.scale : -INFINITY;
        acc[r] = v;
        mi = fmaxf(mi, v);
      }
      mi = fmaxf(mi, __shfl_xor(mi, 32, 64));
      const float m_new = fmaxf(m_run, mi);  // finite: the sub-tile has at least one key
      const float alpha = m_run > -INFINITY ? __expf(m_run - m_new) : 0.f;  // rescale of what the earlier keys left
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = acc[r] > -INFINITY ? __expf(acc[r] - m_new) : 0.f;
        acc[r] = e;
        sum += e;
      }
      sum += __shfl_xor(sum, 32, 64);
      l_run = l_run * alpha + sum;
      m_run = m_new;
      if (p.drop_thresh) {
        const unsigned lo = lo0 + (unsigned)(j * LT + t * 32);
#pragma unroll
        for (int r = 0; r < 16; ++r)
          acc[r] *= lng_keep_lo(lo + (unsigned)((r & 3) + 8 * (r >> 2) + 4 * hh), s0, c2, p.drop_thresh) ? p.drop_inv_keep : 0.f;
      }
      // O^T[dcol][query] = alpha O^T + sum_key V[key][dcol] P[query][key]
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] *= alpha;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        o = __builtin_amdgcn_mfma_f32_32x32x2f32(s.V[key * LLD + l31], acc[r], o, 0, 0, 0);
      }
    }
  }
  if (!active) return;
  const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
  if (hh == 0 && qi < qcnt && p.lse) p.lse[(long)(q_start + q0 + qi) * p.H + h] = m_run + logf(l_run);
  if (qi < qcnt && s.qown[qi]) {
    float* orow = p.out + (long)s.qrow[qi] * p.out_ld + h * d;
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const int dc = 8 * q4 + 4 * hh;
      if (dc < d) st4(orow + dc, make_float4(o[4 * q4] * inv, o[4 * q4 + 1] * inv, o[4 * q4 + 2] * inv, o[4 * q4 + 3] * inv));
    }
  }
}

// ------------------------------------------------------------------------------------ backward: dQ (and delta)
template <bool NORM>
__global__ __launch_bounds__(256, 2) void attn_long_dq_kernel(LngP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  LngSmem s = lng_carve(smem, true);
  __shared__ float lnacc[2][32];
  __shared__ float colred[NORM ? 2 : 1][NORM ? 8 : 1][32];
  const int tid = threadIdx.x, wave = tid >> 6, l31 = tid & 31, hh = (tid >> 5) & 1;
  const int h = blockIdx.y, d = p.d;
  const int* bd = p.blocks + (blockIdx.x / p.slabs) * 6;
  const int q0 = (blockIdx.x % p.slabs) * LT;
  const int first_tile = bd[0], n_tiles = bd[1], tile_step = bd[2];
  const int k_start = bd[4], k_len = min(bd[5], LNG_MAX);
  const int nimg = (k_len + LT - 1) / LT;
  const float sl2 = p.scale * LNG_LOG2E;

  for (int i = tid; i < k_len; i += 256) s.krow[i] = p.kidx ? p.kidx[k_start + i] : k_start + i;
  if (tid < 64) lnacc[tid >> 5][tid & 31] = 0.f;
  if constexpr (NORM) lng_load_affine(p, s);
  const int qi = wave * 32 + l31;  // this lane's query of the slab

  for (int ti = 0; ti < n_tiles; ++ti) {
    const int tile = first_tile + ti * tile_step;
    const int q_start = p.tiles[tile * 4 + 0], q_len = p.tiles[tile * 4 + 1];
    if (q0 >= q_len) continue;
    const int qcnt = min(LT, q_len - q0);
    __syncthreads();  // the previous tile's stores are done with the images
    if (tid < LT) {
      s.qrow[tid] = tid < qcnt ? (p.qidx ? p.qidx[q_start + q0 + tid] : q_start + q0 + tid) : -1;
      s.qown[tid] = tid < qcnt ? (p.owner ? p.owner[q_start + q0 + tid] : 1) : 0;
      s.lse[tid] = tid < qcnt ? p.lse[(long)(q_start + q0 + tid) * p.H + h] * LNG_LOG2E : INFINITY;  // log2 units
    }
    __syncthreads();
    LngStage sk, sv;
    if (k_len > 0) {
      lng_issue(sk, p.kv, p.kv_ld, p.k_off + h * d, s.krow, min(LT, k_len), d);
      lng_issue(sv, p.kv, p.kv_ld, p.v_off + h * d, s.krow, min(LT, k_len), d);
    }
    {  // Q rows, dO rows (zero for non-owners) and delta = rowsum(dO * O)
      const int sub = tid & 7, rr0 = tid >> 3;
      float4 qv[4], gv[4], ov[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = rr0 + 32 * j;
        qv[j] = gv[j] = ov[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < qcnt && sub * 4 < d) {
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
        float* oq = s.Q + r * LLD + sub * 4;
        oq[0] = qv[j].x; oq[1] = qv[j].y; oq[2] = qv[j].z; oq[3] = qv[j].w;
        float* o = s.dO + r * LLD + sub * 4;
        o[0] = gv[j].x; o[1] = gv[j].y; o[2] = gv[j].z; o[3] = gv[j].w;
        float dsum = gv[j].x * ov[j].x + gv[j].y * ov[j].y + gv[j].z * ov[j].z + gv[j].w * ov[j].w;
        dsum += __shfl_xor(dsum, 1, 64);
        dsum += __shfl_xor(dsum, 2, 64);
        dsum += __shfl_xor(dsum, 4, 64);
        if (sub == 0) {
          s.Dv[r] = dsum;
          if (r < qcnt) p.delta[(long)(q_start + q0 + r) * p.H + h] = dsum;
        }
      }
    }
    __syncthreads();
    if constexpr (NORM) {
      if (tid < LT) lng_ln_rows<false>(s.Q, s.qrstd, tid, qcnt, d, p.eps, nullptr, nullptr);
      __syncthreads();
    }
    // this lane's query row (with the norm's affine) and its dO row: the B operands of S^T and dP^T
    float qb[16], gb[16];
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) {
      const int k = 2 * s2 + hh;
      qb[s2] = NORM ? s.Q[qi * LLD + k] * s.gq[k] + s.bq[k] : s.Q[qi * LLD + k];
      gb[s2] = s.dO[qi * LLD + k];
    }
    const float lse_q = s.lse[qi], d_q = s.Dv[qi];
    const bool active = wave * 32 < qcnt;
    f32x16 dq = lng_zero16();
    const unsigned long long rb = ((((unsigned long long)tile * p.H + h) * LNG_MAX) + (unsigned)(q0 + qi)) * LNG_MAX;
    const unsigned lo0 = (unsigned)rb, c2 = (unsigned)(rb >> 32) * 0x7FEB352Du + (unsigned)(p.drop_seed >> 32);
    const unsigned s0 = (unsigned)p.drop_seed;

    for (int j = 0; j < nimg; ++j) {
      const int kcnt = min(LT, k_len - j * LT);
      __syncthreads();  // the previous image's products are done with K and V
      lng_commit(sk, s.K, kcnt, d);
      lng_commit(sv, s.V, kcnt, d);
      __syncthreads();
      if constexpr (NORM) {
        if (tid >= LT) lng_ln_rows<true>(s.K, s.krstd, tid - LT, kcnt, d, p.eps, s.gk, s.bk);
        __syncthreads();
      }
      {  // the next image's rows (the last image once more at the end: no branch around a load)
        const int jn = min(j + 1, nimg - 1), ncnt = min(LT, k_len - jn * LT);
        lng_issue(sk, p.kv, p.kv_ld, p.k_off + h * d, s.krow + jn * LT, ncnt, d);
        lng_issue(sv, p.kv, p.kv_ld, p.v_off + h * d, s.krow + jn * LT, ncnt, d);
      }
      if (!active) continue;
      const int ktiles = (kcnt + 31) / 32;
      for (int t = 0; t < ktiles; ++t) {
        f32x16 sa = lng_zero16(), dpa = lng_zero16();
        const float* krow_p = s.K + (t * 32 + l31) * LLD + hh;
        const float* vrow_p = s.V + (t * 32 + l31) * LLD + hh;
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) {
          sa = __builtin_amdgcn_mfma_f32_32x32x2f32(krow_p[2 * s2], qb[s2], sa, 0, 0, 0);
          dpa = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow_p[2 * s2], gb[s2], dpa, 0, 0, 0);
        }
        const unsigned lo = lo0 + (unsigned)(j * LT + t * 32);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
          const float e = key < kcnt ? __builtin_amdgcn_exp2f(sa[r] * sl2 - lse_q) : 0.f;
          float keep = 1.f;
          if (p.drop_thresh) keep = lng_keep_lo(lo + (unsigned)((r & 3) + 8 * (r >> 2) + 4 * hh), s0, c2, p.drop_thresh) ? p.drop_inv_keep : 0.f;
          const float ds = e * (dpa[r] * keep - d_q) * p.scale;
          // dQ^T[dcol][query] += K[key][dcol] dS[query][key]
          dq = __builtin_amdgcn_mfma_f32_32x32x2f32(s.K[key * LLD + l31], ds, dq, 0, 0, 0);
        }
      }
    }
    __syncthreads();  // every wave holds its dO fragment: the dO image takes dQ
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int dc = (r & 3) + 8 * (r >> 2) + 4 * hh;
      s.dO[qi * LLD + dc] = (dc < d) ? dq[r] : 0.f;
    }
    __syncthreads();
    if constexpr (NORM) {
      const int j = tid & 31, part = tid >> 5;
      float ag = 0.f, ab = 0.f;
      if (j < d)
        for (int r = part * 16; r < min(qcnt, part * 16 + 16); ++r) {
          const float g = s.dO[r * LLD + j];
          ag += g * s.Q[r * LLD + j];
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
      if (tid < LT) lng_ln_rows_bwd(s.dO, s.Q, s.qrstd, tid, qcnt, d, s.gq);
      __syncthreads();
    }
    lng_store_rows(s.dO, p.dq, p.dq_ld, p.dq_off + h * d, s.qrow, s.qown, qcnt, d);
  }
  if constexpr (NORM) {
    __syncthreads();
    if (tid < 64) p.ln_part[((long)(blockIdx.x * p.H + h) * 4 + (tid >> 5)) * 32 + (tid & 31)] = lnacc[tid >> 5][tid & 31];
  }
}

// ------------------------------------------------------------------------------------ backward: dK / dV
template <bool NORM>
__global__ __launch_bounds__(256, 2) void attn_long_dkv_kernel(LngP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  LngSmem s = lng_carve(smem, true);
  __shared__ float colred[NORM ? 2 : 1][NORM ? 8 : 1][32];
  const int tid = threadIdx.x, wave = tid >> 6, l31 = tid & 31, hh = (tid >> 5) & 1;
  const int h = blockIdx.y, d = p.d;
  const int* bd = p.blocks + (blockIdx.x / p.slabs) * 6;
  const int k0 = (blockIdx.x % p.slabs) * LT;
  const int first_tile = bd[0], n_tiles = bd[1], tile_step = bd[2], part_slot = bd[3];
  const int k_start = bd[4], k_len = min(bd[5], LNG_MAX);
  float* ln_out = p.ln_part + ((long)(blockIdx.x * p.H + h) * 4 + 2) * 32;  // dgamma_k | dbeta_k of this (block, head)
  if (k0 >= k_len) {
    if (NORM && tid < 64) ln_out[tid] = 0.f;
    return;
  }
  const int kcnt = min(LT, k_len - k0);
  int* krow = s.krow;
  int* kext = s.krow + LT;
  const float sl2 = p.scale * LNG_LOG2E;

  if (tid < LT) {
    krow[tid] = tid < kcnt ? (p.kidx ? p.kidx[k_start + k0 + tid] : k_start + k0 + tid) : -1;
    kext[tid] = (tid < kcnt && p.kext) ? p.kext[k_start + k0 + tid] : -1;
  }
  if constexpr (NORM) lng_load_affine(p, s);
  __syncthreads();
  {
    LngStage sk, sv;
    lng_issue(sk, p.kv, p.kv_ld, p.k_off + h * d, krow, kcnt, d);
    lng_issue(sv, p.kv, p.kv_ld, p.v_off + h * d, krow, kcnt, d);
    lng_commit(sk, s.K, kcnt, d);
    lng_commit(sv, s.V, kcnt, d);
  }
  __syncthreads();
  if constexpr (NORM) {
    if (tid >= LT) lng_ln_rows<false>(s.K, s.krstd, tid - LT, kcnt, d, p.eps, nullptr, nullptr);
    __syncthreads();
  }
  const int r0 = wave * 32, kj = r0 + l31;  // this lane's key of the image
  const bool has_keys = r0 < kcnt, key_in = kj < kcnt;
  float kb[16], vb[16];
#pragma unroll
  for (int s2 = 0; s2 < 16; ++s2) {
    const int k = 2 * s2 + hh;
    kb[s2] = (NORM ? s.K[kj * LLD + k] * s.gk[k] + s.bk[k] : s.K[kj * LLD + k]) * sl2;
    vb[s2] = s.V[kj * LLD + k];
  }
  const float c_a = key_in ? 0.f : -INFINITY;
  f32x16 acc_dv = lng_zero16(), acc_dk = lng_zero16();

  for (int ti = 0; ti < n_tiles; ++ti) {
    const int tile = first_tile + ti * tile_step;
    const int q_start = p.tiles[tile * 4 + 0], q_len = min(p.tiles[tile * 4 + 1], p.slabs * LT);
    const unsigned long long tb = (((unsigned long long)tile * p.H + h) * LNG_MAX) * LNG_MAX;
    const unsigned c2 = (unsigned)(tb >> 32) * 0x7FEB352Du + (unsigned)(p.drop_seed >> 32);
    const unsigned s0 = (unsigned)p.drop_seed;
    for (int q0 = 0; q0 < q_len; q0 += LT) {
      const int qcnt = min(LT, q_len - q0);
      __syncthreads();  // the previous slab's products are done with Q, dO and the row scalars
      if (tid < LT) {
        s.qrow[tid] = tid < qcnt ? (p.qidx ? p.qidx[q_start + q0 + tid] : q_start + q0 + tid) : -1;
        s.qown[tid] = tid < qcnt ? (p.owner ? p.owner[q_start + q0 + tid] : 1) : 0;
        s.lse[tid] = tid < qcnt ? p.lse[(long)(q_start + q0 + tid) * p.H + h] * LNG_LOG2E : INFINITY;  // log2 units
        s.Dv[tid] = tid < qcnt ? p.delta[(long)(q_start + q0 + tid) * p.H + h] : 0.f;
      }
      __syncthreads();
      {  // Q rows and dO rows (zero for non-owners)
        const int sub = tid & 7, rr0 = tid >> 3;
        float4 qv[4], gv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = rr0 + 32 * j;
          qv[j] = gv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (r < qcnt && sub * 4 < d) {
            qv[j] = ld4(p.q + (long)s.qrow[r] * p.q_ld + p.q_off + h * d + sub * 4);
            if (s.qown[r]) gv[j] = ld4(p.dout + (long)s.qrow[r] * p.out_ld + h * d + sub * 4);
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = rr0 + 32 * j;
          float* oq = s.Q + r * LLD + sub * 4;
          oq[0] = qv[j].x; oq[1] = qv[j].y; oq[2] = qv[j].z; oq[3] = qv[j].w;
          float* o = s.dO + r * LLD + sub * 4;
          o[0] = gv[j].x; o[1] = gv[j].y; o[2] = gv[j].z; o[3] = gv[j].w;
        }
      }
      __syncthreads();
      if constexpr (NORM) {
        if (tid < LT) lng_ln_rows<true>(s.Q, s.qrstd, tid, qcnt, d, p.eps, s.gq, s.bq);
        __syncthreads();
      }
      if (!has_keys) continue;
      const int qtiles = (qcnt + 31) / 32;
      for (int qt = 0; qt < qtiles; ++qt) {
        f32x16 sa, dpa;
#pragma unroll
        for (int r = 0; r < 16; ++r) { sa[r] = c_a; dpa[r] = 0.f; }
        const float* qrow_p = s.Q + (qt * 32 + l31) * LLD + hh;
        const float* dorow_p = s.dO + (qt * 32 + l31) * LLD + hh;
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
        // element (query q0 + qq, key k0 + kj) of the tile: low word of idx
        const unsigned lo_k = (unsigned)tb + (unsigned)(k0 + kj) + (unsigned)((q0 + qt * 32 + 4 * hh) * LNG_MAX);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float e = __builtin_amdgcn_exp2f(sa[r] - lse4[r]);
          float keep = 1.f;
          if (p.drop_thresh) keep = lng_keep_lo(lo_k + (unsigned)(((r & 3) + 8 * (r >> 2)) * LNG_MAX), s0, c2, p.drop_thresh) ? p.drop_inv_keep : 0.f;
          sa[r] = e * keep;                                    // dropout(P)
          dpa[r] = e * (dpa[r] * keep - d4[r]) * p.scale;      // dS
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int qq = qt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
          acc_dv = __builtin_amdgcn_mfma_f32_32x32x2f32(s.dO[qq * LLD + l31], sa[r], acc_dv, 0, 0, 0);
          acc_dk = __builtin_amdgcn_mfma_f32_32x32x2f32(s.Q[qq * LLD + l31], dpa[r], acc_dk, 0, 0, 0);
        }
      }
    }
  }
  __syncthreads();  // every wave is done with the images: V takes dV, dO takes dK
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int dc = (r & 3) + 8 * (r >> 2) + 4 * hh;
    s.V[kj * LLD + dc] = (dc < d) ? acc_dv[r] : 0.f;
    s.dO[kj * LLD + dc] = (dc < d) ? acc_dk[r] : 0.f;
  }
  __syncthreads();
  if constexpr (NORM) {
    const int j = tid & 31, part = tid >> 5;
    float ag = 0.f, ab = 0.f;
    if (j < d)
      for (int r = part * 16; r < min(kcnt, part * 16 + 16); ++r) {
        const float g = s.dO[r * LLD + j];
        ag += g * s.K[r * LLD + j];
        ab += g;
      }
    colred[0][part][j] = ag;
    colred[1][part][j] = ab;
    __syncthreads();
    if (tid < 64) {
      const int which = tid >> 5, j2 = tid & 31;  // dgamma_k, dbeta_k
      float a = 0.f;
      for (int k = 0; k < 8; ++k) a += colred[which][k][j2];
      ln_out[which * 32 + j2] = a;
    }
    if (tid < LT) lng_ln_rows_bwd(s.dO, s.K, s.krstd, tid, kcnt, d, s.gk);
    __syncthreads();
  }
  float* dkv = p.dkv + (long)part_slot * p.dkv_part_stride;
  lng_store_rows(s.dO, dkv, p.dkv_ld, p.dk_off + h * d, krow, nullptr, kcnt, d, p.dkv_extra ? kext : nullptr, p.dkv_extra,
                 p.dkv_extra_ld, h * d);
  lng_store_rows(s.V, dkv, p.dkv_ld, p.dv_off + h * d, krow, nullptr, kcnt, d, p.dkv_extra ? kext : nullptr, p.dkv_extra,
                 p.dkv_extra_ld, p.dv_off - p.dk_off + h * d);
}

// out[which][j] (+)= sum over the (block, head) partial rows, ascending, in float64
__global__ __launch_bounds__(128) void attn_long_ln_reduce_kernel(const float* __restrict__ part, float* o0, float* o1, float* o2,
                                                                  float* o3, int nparts, int d, int accumulate) {
  const int which = threadIdx.x >> 5, j = threadIdx.x & 31;
  if (j >= d) return;
  double sum = 0.0;
  for (int b = 0; b < nparts; ++b) sum += (double)part[((long)b * 4 + which) * 32 + j];
  float* o = which == 0 ? o0 : which == 1 ? o1 : which == 2 ? o2 : o3;
  o[j] = accumulate ? (float)((double)o[j] + sum) : (float)sum;
}

// dqkv[point][k|v columns] += extra[e] for every borrowed copy e (each point is borrowed at most once)
__global__ void attn_long_extra_fixup_kernel(const float* __restrict__ extra, long extra_ld, const int* __restrict__ ext_pos,
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

static void lng_set_drop(LngP& p, float drop_p, unsigned long long seed) {
  p.drop_seed = seed;
  p.drop_thresh = 0;
  p.drop_inv_keep = 1.f;
  if (drop_p > 0.f) {
    p.drop_thresh = (unsigned)(drop_p * 4294967296.0);
    if (p.drop_thresh == 0) p.drop_thresh = 1;
    p.drop_inv_keep = 1.f / (1.f - drop_p);
  }
}

static int lng_norm_mode(const float* qn_w, const float* qn_b, const float* kn_w, const float* kn_b) {
  const int n = (qn_w != nullptr) + (qn_b != nullptr) + (kn_w != nullptr) + (kn_b != nullptr);
  return n == 4 ? 1 : n == 0 ? 0 : -1;
}

// what both entry points refuse alike
static int lng_check(const char* who, int H, int d, int len_max, float drop_p) {
  LOTUS_CHECK_ARG(H > 0 && d >= 4 && d <= 32 && d % 4 == 0, "%s: H = %d, d = %d (H > 0; d a multiple of 4 up to 32)", who, H, d);
  LOTUS_CHECK_ARG(len_max >= 1, "%s: len_max = %d must be at least 1 (the longest q_len / k_len of a tile)", who, len_max);
  LOTUS_CHECK_ARG(len_max <= LNG_MAX, "%s: len_max = %d > %d (a tile of the long kernels has at most that many queries and keys)",
                  who, len_max, LNG_MAX);
  LOTUS_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "%s: drop_p = %g outside [0, 1)", who, (double)drop_p);
  return LOTUS_OK;
}

extern "C" {

int lotus_attention_long_fwd(const float* q, long q_ld, int q_off, const float* kv, long kv_ld, int k_off, int v_off, const int* qidx,
                             const int* kidx, const int* owner, const int* tiles, int ntiles, const float* qn_w, const float* qn_b,
                             const float* kn_w, const float* kn_b, float* out, long out_ld, float* lse, int H, int d, float scale,
                             float eps, float drop_p, unsigned long long drop_seed, int len_max, void* stream) {
  LOTUS_CHECK_ARG(q && kv && tiles && out, "lotus_attention_long_fwd: null pointer (q, kv, tiles, out)");
  const int rc = lng_check("lotus_attention_long_fwd", H, d, len_max, drop_p);
  if (rc) return rc;
  const int norm = lng_norm_mode(qn_w, qn_b, kn_w, kn_b);
  LOTUS_CHECK_ARG(norm >= 0, "lotus_attention_long_fwd: qn_w, qn_b, kn_w, kn_b must be all given or all null");
  LOTUS_CHECK_ARG(ntiles >= 0, "lotus_attention_long_fwd: ntiles = %d must not be negative", ntiles);
  if (ntiles == 0) return LOTUS_OK;
  LngP p;
  memset(&p, 0, sizeof(p));
  p.q = q; p.q_ld = q_ld; p.q_off = q_off; p.kv = kv; p.kv_ld = kv_ld; p.k_off = k_off; p.v_off = v_off;
  p.qidx = qidx; p.kidx = kidx; p.owner = owner; p.tiles = tiles;
  p.qn_w = qn_w; p.qn_b = qn_b; p.kn_w = kn_w; p.kn_b = kn_b;
  p.out = out; p.out_ld = out_ld; p.lse = lse; p.H = H; p.d = d; p.scale = scale; p.eps = eps;
  p.slabs = cdiv(len_max, LT);
  lng_set_drop(p, drop_p, drop_seed);
  const size_t lds = lng_smem_bytes(false);
  lotus_note_attn_route(LOTUS_ATTN_LONG_FWD, 0, 0, 0, norm, 256, (int)lds, 0);
  const dim3 g((unsigned)ntiles * p.slabs, H), b(256);
  if (norm) {
    lotus_allow_dyn_lds_once<attn_long_fwd_kernel<true>>(lds);
    LOTUS_LAUNCH(attn_long_fwd_kernel<true>, g, b, lds, (hipStream_t)stream, p);
  } else {
    lotus_allow_dyn_lds_once<attn_long_fwd_kernel<false>>(lds);
    LOTUS_LAUNCH(attn_long_fwd_kernel<false>, g, b, lds, (hipStream_t)stream, p);
  }
  LOTUS_LAUNCH_CHECK("lotus_attention_long_fwd");
  return LOTUS_OK;
}

size_t lotus_attention_long_bwd_workspace(int nblocks, int H, int len_max, long npos) {
  if (nblocks < 0 || H <= 0 || len_max < 1 || len_max > LNG_MAX || npos < 0) return 0;
  const size_t delta = ((size_t)npos * H + 3) / 4 * 4;
  return (delta + (size_t)nblocks * cdiv(len_max, LT) * H * 4 * 32) * sizeof(float);
}

int lotus_attention_long_bwd(const float* q, long q_ld, int q_off, const float* kv, long kv_ld, int k_off, int v_off, const int* qidx,
                             const int* kidx, const int* owner, const int* tiles, const int* blocks, int nblocks, const float* qn_w,
                             const float* qn_b, const float* kn_w, const float* kn_b, const float* out, const float* dout, long out_ld,
                             const float* lse, float* dq, long dq_ld, int dq_off, float* dkv, long dkv_ld, int dk_off, int dv_off,
                             long dkv_part_stride, const int* kext, const int* ext_pos, int n_extra, float* dkv_extra, float* dqn_w,
                             float* dqn_b, float* dkn_w, float* dkn_b, int accumulate, int H, int d, float scale, float eps, float drop_p,
                             unsigned long long drop_seed, int len_max, long npos, void* workspace, size_t workspace_bytes,
                             void* stream) {
  LOTUS_CHECK_ARG(q && kv && tiles && blocks && out && dout && lse && dq && dkv,
                  "lotus_attention_long_bwd: null pointer (q, kv, tiles, blocks, out, dout, lse, dq, dkv)");
  const int rc = lng_check("lotus_attention_long_bwd", H, d, len_max, drop_p);
  if (rc) return rc;
  const int norm = lng_norm_mode(qn_w, qn_b, kn_w, kn_b);
  LOTUS_CHECK_ARG(norm >= 0, "lotus_attention_long_bwd: qn_w, qn_b, kn_w, kn_b must be all given or all null");
  LOTUS_CHECK_ARG(!norm || (dqn_w && dqn_b && dkn_w && dkn_b), "lotus_attention_long_bwd: null norm gradient");
  LOTUS_CHECK_ARG(nblocks >= 0, "lotus_attention_long_bwd: nblocks = %d must not be negative", nblocks);
  LOTUS_CHECK_ARG(npos >= 0, "lotus_attention_long_bwd: npos = %ld must not be negative (rows of lse)", npos);
  LOTUS_CHECK_ARG(nblocks == 0 || (workspace && ((uintptr_t)workspace) % 8 == 0 &&
                                   workspace_bytes >= lotus_attention_long_bwd_workspace(nblocks, H, len_max, npos)),
                  "lotus_attention_long_bwd: workspace too small or misaligned (lotus_attention_long_bwd_workspace(nblocks, H, "
                  "len_max, npos) bytes, 8-byte aligned)");
  const bool extra = kext && n_extra > 0;
  LOTUS_CHECK_ARG(!extra || (dkv_extra && ext_pos && kidx && dv_off - dk_off == H * d),
                  "lotus_attention_long_bwd: borrowed-row buffer needs dkv_extra, ext_pos, kidx and adjacent k|v column blocks");
  if (nblocks == 0) return LOTUS_OK;
  hipStream_t st = (hipStream_t)stream;
  StopEventOnLast stop_ev;
  LngP p;
  memset(&p, 0, sizeof(p));
  p.q = q; p.q_ld = q_ld; p.q_off = q_off; p.kv = kv; p.kv_ld = kv_ld; p.k_off = k_off; p.v_off = v_off;
  p.qidx = qidx; p.kidx = kidx; p.owner = owner; p.tiles = tiles; p.blocks = blocks;
  p.qn_w = qn_w; p.qn_b = qn_b; p.kn_w = kn_w; p.kn_b = kn_b;
  p.out = (float*)out; p.dout = dout; p.out_ld = out_ld; p.lse = (float*)lse;
  p.dq = dq; p.dq_ld = dq_ld; p.dq_off = dq_off;
  p.dkv = dkv; p.dkv_ld = dkv_ld; p.dk_off = dk_off; p.dv_off = dv_off; p.dkv_part_stride = dkv_part_stride;
  p.slabs = cdiv(len_max, LT);
  p.delta = (float*)workspace;
  p.ln_part = (float*)workspace + ((size_t)npos * H + 3) / 4 * 4;
  p.kext = kext; p.dkv_extra = extra ? dkv_extra : nullptr; p.dkv_extra_ld = 2L * H * d;
  p.H = H; p.d = d; p.scale = scale; p.eps = eps;
  lng_set_drop(p, drop_p, drop_seed);
  const size_t lds = lng_smem_bytes(true);
  const int tail = (extra ? LOTUS_ATTN_TAIL_FIXUP : 0) | (norm ? LOTUS_ATTN_TAIL_LN_REDUCE : 0);
  lotus_note_attn_route(LOTUS_ATTN_LONG_BWD, 1, 0, 0, norm, 256, (int)lds, tail);
  const dim3 g((unsigned)nblocks * p.slabs, H), b(256);
  if (norm) {
    lotus_allow_dyn_lds_once<attn_long_dq_kernel<true>>(lds);
    lotus_allow_dyn_lds_once<attn_long_dkv_kernel<true>>(lds);
    LOTUS_LAUNCH(attn_long_dq_kernel<true>, g, b, lds, st, p);
    if (!tail) stop_ev.last();
    LOTUS_LAUNCH(attn_long_dkv_kernel<true>, g, b, lds, st, p);
  } else {
    lotus_allow_dyn_lds_once<attn_long_dq_kernel<false>>(lds);
    lotus_allow_dyn_lds_once<attn_long_dkv_kernel<false>>(lds);
    LOTUS_LAUNCH(attn_long_dq_kernel<false>, g, b, lds, st, p);
    if (!tail) stop_ev.last();
    LOTUS_LAUNCH(attn_long_dkv_kernel<false>, g, b, lds, st, p);
  }
  if (extra) {
    const int w4 = 2 * H * d / 4;
    if (!norm) stop_ev.last();
    LOTUS_LAUNCH(attn_long_extra_fixup_kernel, dim3(cdiv((long)n_extra * w4, 256)), dim3(256), 0, st, (const float*)dkv_extra,
                 2L * H * d, ext_pos, kidx, n_extra, w4, dkv, dkv_ld, dk_off);
  }
  if (norm) {
    stop_ev.last();
    LOTUS_LAUNCH(attn_long_ln_reduce_kernel, dim3(1), dim3(128), 0, st, (const float*)p.ln_part, dqn_w, dqn_b, dkn_w, dkn_b,
                 nblocks * p.slabs * H, d, accumulate);
  }
  LOTUS_LAUNCH_CHECK("lotus_attention_long_bwd");
  return LOTUS_OK;
}

}  // extern "C"

}  // namespace LOTUS_NS
