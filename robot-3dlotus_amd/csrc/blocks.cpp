// lotus-hip: composite entry points — one C call enqueues the whole forward or backward of a transformer sub-block.
//
// The Python host used to issue the 3-11 launches of a sub-block one C-ABI call at a time (allocation, argument
// conversion and bookkeeping per launch: ~8 us of interpreter time each, ~1000 launches per step).  These functions
// chain the SAME entry points in the SAME order on the same streams, so results are bit-identical to the per-launch
// path (tests/test_gpu_blocks.py); the host allocates three flat buffers per call (saved activations, gradients,
// temporaries) whose layouts are defined here.
//
// Weight gradients go to `side` (0 = same stream as everything else) after `lotus_streamlink_wait(link, main, side)`,
// exactly like ops._OnSide; join != 0 orders `main` after `side` at the end (ops "node" join mode).
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../../include/lotus_hip.h"

extern __attribute__((visibility("hidden"))) __thread hipEvent_t lotus_tls_stop_event;  // common.h: LOTUS_LAUNCH
hipEvent_t lotus_link_next_event(unsigned long long link);  // lotus_capi.cpp
void lotus_set_error(const char* fmt, ...);

#define CHECK(x)        \
  do {                  \
    int rc_ = (x);      \
    if (rc_) return rc_; \
  } while (0)

// This file is compiled twice (act_t = float and act_t = bf16) into one library: everything that is not an entry point
// has internal linkage, or the linker would keep one build's copy of a layout constructor for both.
namespace {

static inline size_t al4(size_t n) { return (n + 3) & ~(size_t)3; }  // keep every slice 16-byte aligned

// Activation element type of this build (include/lotus_hip.h: float, or 16-bit bf16 storage in the lotus_b16_* twin).  The
// flat `saved` / `tmp` buffers are carved in bytes: activation slices take n * sizeof(act_t), statistics n * 4, each rounded
// up to 16 bytes; their sizes are still reported in floats (the host allocates fp32 words).  In the fp32 build the
// layout is what it always was.
typedef lotus_act_t act_t;
static inline size_t actf(size_t n) { return al4((n * sizeof(act_t) + 3) / 4); }  // floats holding n activations

// Parameter gradients in slab order, (offset, length) in floats: what lotus_composite_grads_layout reports.
struct Fields {
  long long *off, *len;
  int cap, n;
};

// The one place that puts slices into a flat buffer: a region of `slab` that begins at float `start` (`base`) and ends
// before float `end`, which moves on with every slice taken.  `slab` may be null (size queries: only `end` means something).
// The layout structs below derive from it and take their named slices in their constructors.
struct Carve {
  float *slab, *base;
  size_t end;
  Fields* rec;
  Carve(const float* slab_, size_t start, Fields* rec_ = nullptr) : slab((float*)slab_), end(start), rec(rec_) { base = here(); }
  float* here() const { return slab ? slab + end : nullptr; }
  act_t* act(size_t k) { act_t* r = (act_t*)here(); end += actf(k); return r; }
  float* f32(size_t k) { float* r = here(); end = al4(end + k); return r; }
  // column partials of a LayerNorm backward: the tail of a tmp buffer, taken whole (not rounded)
  float* ln_partials(int M, int C, size_t* bytes) {
    float* r = here();
    *bytes = lotus_layernorm_bwd_workspace(M, C);
    end += *bytes / sizeof(float);
    return r;
  }
  // parameter gradients: a weight is followed by its bias without a gap (dw | db), every other field starts on 16 bytes
  float* weight(size_t k) { note(k); float* r = here(); end += k; return r; }
  float* vec(size_t k) { note(k); return f32(k); }
  void note(size_t k) {
    if (!rec) return;
    if (rec->n < rec->cap) rec->off[rec->n] = (long long)end, rec->len[rec->n] = (long long)k;
    ++rec->n;
  }
};

// precision 5 = bf16 products with the LINEAR layers' weights given as bf16 shadows (bf16-storage build, gemm.hip); the
// attention and convolution entry points have no such operand and take the plain code
static inline int noshadow(int precision) { return precision == 5 ? 1 : precision; }

static inline int fork_side(unsigned long long link, void* main_s, void* side) {
  return side ? lotus_streamlink_wait(link, main_s, side) : 0;
}

// Fork bound to a producer: the kernels enqueued while a ForkAfter lives carry one of the link's events as their stop
// event (the last launch wins, like re-recording), and wait() orders `side` after it.  Unlike fork_side() this puts no
// event-record marker between the producer and the next kernel of the critical stream.
struct ForkAfter {
  hipEvent_t ev;
  void* side;
  ForkAfter(unsigned long long link, void* side_) : ev(side_ ? lotus_link_next_event(link) : nullptr), side(side_) {
    lotus_tls_stop_event = ev;
  }
  ~ForkAfter() { lotus_tls_stop_event = nullptr; }
  int wait() {
    lotus_tls_stop_event = nullptr;
    if (!side) return 0;
    hipError_t e = hipStreamWaitEvent((hipStream_t)side, ev, 0);
    if (e != hipSuccess) {
      lotus_set_error("lotus composite: hipStreamWaitEvent: %s", hipGetErrorString(e));
      return LOTUS_E_LAUNCH;
    }
    return 0;
  }
};
#define PRODUCE_THEN_FORK(call) \
  do {                          \
    ForkAfter fa_(link, side);  \
    CHECK(call);                \
    CHECK(fa_.wait());          \
  } while (0)

// What a stream's launches may use besides the stream: a split-K workspace and its counters.
struct Ws {
  void* p;
  size_t bytes;
  void* counters;
};
// The main workspace is offered only to layers of at most 8192 rows (M <= 8192): the per-launch path only offers a split-K
// workspace to the small-M layers, and the composites must pick the same kernels.
static inline Ws small_rows_only(Ws w, int rows) { return rows > 8192 ? Ws{nullptr, 0, nullptr} : w; }
// Where the weight gradients go: the side stream with its own workspace, or (side == 0) the critical stream with the main one.
struct WgradLane {
  void* stream;
  Ws ws;
  WgradLane(void* side, const Ws& ws_side, void* main_s, const Ws& ws_main) : stream(side ? side : main_s), ws(side ? ws_side : ws_main) {}
};

// *dz = dy times the dropout mask (p, seed) of this sub-block's output, with the weight-gradient stream ordered after it.
static int masked_dy(const act_t* dy, const act_t* dz_in, act_t* buf, long n, float p, unsigned long long seed, unsigned long long link,
                     void* stream, void* side, const act_t** dz) {
  // dz_in was written by the LayerNorm backward of the sub-block that ran just before this one, and the weight-gradient
  // stream is already ordered after that launch (its parameter-gradient reduction waited for it): no fork needed
  if (dz_in) {
    *dz = dz_in;
  } else if (p > 0.f) {
    PRODUCE_THEN_FORK(lotus_dropout(dy, buf, n, p, seed, stream));
    *dz = buf;
  } else {
    *dz = dy;
    CHECK(fork_side(link, stream, side));
  }
  return LOTUS_OK;
}

// The input gradient of the layer that reads a LayerNorm's output + that LayerNorm's backward (lotus_linear_dgrad_ln: ONE
// kernel on the many-row levels with C <= 128, else the product into `dn` and lotus_layernorm_bwd); the column partials of
// dgamma / dbeta are reduced on the weight-gradient stream when there is one.
static int dgrad_ln(const act_t* dyl, const float* w, act_t* dn, const act_t* x, const float* mean, const float* rstd, const float* g,
                    const act_t* add, act_t* dx, act_t* dz, float dz_p, unsigned long long dz_seed, float* dg, float* db, int M, int N,
                    int C, int precision, const Ws& ws, float* lnp, size_t lnp_bytes, unsigned long long link, void* stream,
                    void* side) {
  int nparts = 0;
  act_t* dzo = dz_p > 0.f ? dz : nullptr;
  if (side) {
    PRODUCE_THEN_FORK(lotus_linear_dgrad_ln(dyl, w, x, mean, rstd, g, add, dx, dn, dzo, dz_p, dz_seed, M, N, C, precision, ws.p, ws.bytes,
                                            ws.counters, lnp, lnp_bytes, &nparts, stream));
    CHECK(lotus_layernorm_bwd_params_n(lnp, nparts, C, dg, db, 0, side));
  } else {
    CHECK(lotus_linear_dgrad_ln(dyl, w, x, mean, rstd, g, add, dx, dn, dzo, dz_p, dz_seed, M, N, C, precision, ws.p, ws.bytes, ws.counters,
                                lnp, lnp_bytes, &nparts, stream));
    CHECK(lotus_layernorm_bwd_params_n(lnp, nparts, C, dg, db, 0, stream));
  }
  return LOTUS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Buffer layouts.  One struct per sub-block kind and buffer: the constructor takes the named slices of `slab` from float
// `start` on; with start 0, `end` is what the *_floats query reports.  The size queries, the forward, the backward, the pair
// and lotus_composite_grads_layout all construct these structs; nothing else in this file computes an offset.
//
// MLP sub-block: y = x + drop(fc2(drop(GELU(fc1(LN(x))))))   (PointTransformerV3/model.py:577-583, :669-673)
struct FfnSaved : Carve {  // [n M*C | hpre M*Hd | a M*Hd | mean M | rstd M]
  act_t *n, *hpre, *a;
  float *mean, *rstd;
  FfnSaved(const float* slab, size_t start, int M, int C, int Hd) : Carve(slab, start) {
    n = act((size_t)M * C), hpre = act((size_t)M * Hd), a = act((size_t)M * Hd), mean = f32(M), rstd = f32(M);
  }
};
struct FfnGrads : Carve {  // [dg C | db C | dw1 Hd*C + db1 Hd | dw2 C*Hd + db2 C]
  float *dg, *db, *dw1, *db1, *dw2, *db2;
  FfnGrads(float* slab, size_t start, int C, int Hd, Fields* rec = nullptr) : Carve(slab, start, rec) {
    dg = vec(C), db = vec(C), dw1 = weight((size_t)Hd * C), db1 = vec(Hd), dw2 = weight((size_t)C * Hd), db2 = vec(C);
  }
};
struct FfnTmp : Carve {  // [dz M*C | dh M*Hd | dn M*C | ln partials]; dz = dy times the fc2 dropout mask (computed here or handed over)
  act_t *dz, *dh, *dn;
  float* lnp;
  size_t lnp_bytes;
  FfnTmp(float* slab, size_t start, int M, int C, int Hd) : Carve(slab, start) {
    dz = act((size_t)M * C), dh = act((size_t)M * Hd), dn = act((size_t)M * C), lnp = ln_partials(M, C, &lnp_bytes);
  }
};

// Patch self-attention sub-block: y = x + drop(proj(PatchAttention(qkv(LN(x)))))   (model.py:468-557, :664-667)
struct SelfSaved : Carve {  // [n M*C | qkv M*3C | att M*C | lse npad*H | mean M | rstd M]
  act_t *n, *qkv, *att;
  float *lse, *mean, *rstd;
  SelfSaved(const float* slab, size_t start, int M, int C, int H, int npad) : Carve(slab, start) {
    n = act((size_t)M * C), qkv = act((size_t)M * 3 * C), att = act((size_t)M * C), lse = f32((size_t)npad * H);
    mean = f32(M), rstd = f32(M);
  }
};
struct SelfGrads : Carve {  // [dg C | db C | dwqkv 3C*C + dbqkv 3C | gq d | bq d | gk d | bk d | dwp C*C + dbp C]   (d = C / H)
  float *dg, *db, *dwqkv, *dbqkv, *gq, *bq, *gk, *bk, *dwp, *dbp;
  SelfGrads(float* slab, size_t start, int C, int H, Fields* rec = nullptr) : Carve(slab, start, rec) {
    const int d = C / H;
    dg = vec(C), db = vec(C), dwqkv = weight((size_t)3 * C * C), dbqkv = vec(3 * C);
    gq = vec(d), bq = vec(d), gk = vec(d), bk = vec(d), dwp = weight((size_t)C * C), dbp = vec(C);
  }
};
struct SelfTmp : Carve {  // [dz M*C | datt M*C | dqkv M*3C | extra max(n_extra,1)*2C | dn M*C | ln partials]
  act_t *dz, *datt, *dqkv, *extra, *dn;
  float* lnp;
  size_t lnp_bytes;
  SelfTmp(float* slab, size_t start, int M, int C, int n_extra) : Carve(slab, start) {
    dz = act((size_t)M * C), datt = act((size_t)M * C), dqkv = act((size_t)M * 3 * C);
    extra = act((size_t)(n_extra > 1 ? n_extra : 1) * 2 * C), dn = act((size_t)M * C), lnp = ln_partials(M, C, &lnp_bytes);
  }
};

// Cross-attention sub-block: y = x + drop(proj(CrossAttention(q(LN(x)), kv(context))))   (model_ca.py:46-101, :135-140)
struct CrossSaved : Carve {  // [n M*C | q M*C | kv L*2C | att M*C | lse M*H | mean M | rstd M]
  act_t *n, *q, *kv, *att;
  float *lse, *mean, *rstd;
  CrossSaved(const float* slab, size_t start, int M, int C, int H, int L) : Carve(slab, start) {
    n = act((size_t)M * C), q = act((size_t)M * C), kv = act((size_t)L * 2 * C), att = act((size_t)M * C);
    lse = f32((size_t)M * H), mean = f32(M), rstd = f32(M);
  }
};
struct CrossGrads : Carve {  // [dg C | db C | dwq C*C + dbq C | dwkv 2C*Cc + dbkv 2C | gq d | bq d | gk d | bk d | dwp C*C + dbp C]
  float *dg, *db, *dwq, *dbq, *dwkv, *dbkv, *gq, *bq, *gk, *bk, *dwp, *dbp;
  CrossGrads(float* slab, size_t start, int C, int H, int Cc, Fields* rec = nullptr) : Carve(slab, start, rec) {
    const int d = C / H;
    dg = vec(C), db = vec(C), dwq = weight((size_t)C * C), dbq = vec(C), dwkv = weight((size_t)2 * C * Cc), dbkv = vec(2 * C);
    gq = vec(d), bq = vec(d), gk = vec(d), bk = vec(d), dwp = weight((size_t)C * C), dbp = vec(C);
  }
};
struct CrossTmp : Carve {  // [dz M*C | datt M*C | dq M*C | dkv_part G*L*2C | dkv L*2C | dn M*C | ln partials]
  act_t *dz, *datt, *dq, *dkv_part, *dkv, *dn;
  float* lnp;
  size_t lnp_bytes;
  CrossTmp(float* slab, size_t start, int M, int C, int L, int G) : Carve(slab, start) {
    dz = act((size_t)M * C), datt = act((size_t)M * C), dq = act((size_t)M * C), dkv_part = act((size_t)G * L * 2 * C);
    dkv = act((size_t)L * 2 * C), dn = act((size_t)M * C), lnp = ln_partials(M, C, &lnp_bytes);
  }
};

// Cross-attention sub-block with PRECOMPUTED keys / values (lotus_crossattn_kv_*, below)
struct CrossKvSaved : Carve {  // [n M*C | q M*C | att M*C | lse M*H | mean M | rstd M]
  act_t *n, *q, *att;
  float *lse, *mean, *rstd;
  CrossKvSaved(const float* slab, size_t start, int M, int C, int H) : Carve(slab, start) {
    n = act((size_t)M * C), q = act((size_t)M * C), att = act((size_t)M * C), lse = f32((size_t)M * H), mean = f32(M), rstd = f32(M);
  }
};
struct CrossKvGrads : Carve {  // [dg C | db C | dwq C*C + dbq C | gq d | bq d | gk d | bk d | dwp C*C + dbp C]
  float *dg, *db, *dwq, *dbq, *gq, *bq, *gk, *bk, *dwp, *dbp;
  CrossKvGrads(float* slab, size_t start, int C, int H, Fields* rec = nullptr) : Carve(slab, start, rec) {
    const int d = C / H;
    dg = vec(C), db = vec(C), dwq = weight((size_t)C * C), dbq = vec(C), gq = vec(d), bq = vec(d), gk = vec(d), bk = vec(d);
    dwp = weight((size_t)C * C), dbp = vec(C);
  }
};
struct CrossKvTmp : Carve {  // [dz M*C | datt M*C | dq M*C | dkv_part (G > 1 ? G : 0)*L*2C | dn M*C | ln partials]
  act_t *dz, *datt, *dq, *dkv_part, *dn;
  float* lnp;
  size_t lnp_bytes;
  CrossKvTmp(float* slab, size_t start, int M, int C, int L, int G) : Carve(slab, start) {
    dz = act((size_t)M * C), datt = act((size_t)M * C), dq = act((size_t)M * C), dkv_part = G > 1 ? act((size_t)G * L * 2 * C) : nullptr;
    dn = act((size_t)M * C), lnp = ln_partials(M, C, &lnp_bytes);
  }
};

// Conditional positional encoding: y = x + LN(Linear(SubMConv3d_3(xs)))   (model.py:615-625, :660-662)
struct CpeSaved : Carve {  // [c n*C | l n*C | mean n | rstd n]
  act_t *c, *l;
  float *mean, *rstd;
  CpeSaved(const float* slab, size_t start, int n, int C) : Carve(slab, start) {
    c = act((size_t)n * C), l = act((size_t)n * C), mean = f32(n), rstd = f32(n);
  }
};
struct CpeGrads : Carve {  // [dg C | db C | dlw C*C + dlb C | dcw C*27*C + dcb C]
  float *dg, *db, *dlw, *dlb, *dcw, *dcb;
  CpeGrads(float* slab, size_t start, int C, Fields* rec = nullptr) : Carve(slab, start, rec) {
    dg = vec(C), db = vec(C), dlw = weight((size_t)C * C), dlb = vec(C), dcw = weight((size_t)C * 27 * C), dcb = vec(C);
  }
};
struct CpeTmp : Carve {  // [dl n*C | dc n*C | dyr n*C | ln partials]
  act_t *dl, *dc, *dyr;
  float* lnp;
  size_t lnp_bytes;
  CpeTmp(float* slab, size_t start, int n, int C) : Carve(slab, start) {
    dl = act((size_t)n * C), dc = act((size_t)n * C), dyr = act((size_t)n * C), lnp = ln_partials(n, C, &lnp_bytes);
  }
};

// One (Block, CABlock) pair: the five sub-layouts back to back (cpe, self, ffn1, cross_kv, ffn2).
// Every sub-block's region of the flat saved / tmp buffers starts on a 256-byte boundary: the regions end with per-row
// statistics (M floats), and a following activation slab that is only 16-byte aligned makes every 128-byte row piece the
// attention kernels fetch straddle two cache lines (measured: -1.4 % on the whole step before this rounding).
static inline size_t al64(size_t n) { return (n + 63) & ~(size_t)63; }
struct PairActs : Carve {  // [x1 | x2 | x3 | x4]: outputs of the first four sub-blocks, kept for backward
  act_t* x[4];
  PairActs(const float* slab, size_t start, int M, int C) : Carve(slab, start) {
    for (int i = 0; i < 4; ++i) x[i] = act((size_t)M * C), end = al64(end);
  }
};
struct PairSaved {
  CpeSaved cpe;
  SelfSaved self;
  FfnSaved ffn1;
  CrossKvSaved cross;
  FfnSaved ffn2;
  size_t end;
  PairSaved(const float* slab, int M, int C, int H, int Hd, int npad)
      : cpe(slab, 0, M, C), self(slab, al64(cpe.end), M, C, H, npad), ffn1(slab, al64(self.end), M, C, Hd),
        cross(slab, al64(ffn1.end), M, C, H), ffn2(slab, al64(cross.end), M, C, Hd), end(al64(ffn2.end)) {}
};
struct PairGrads {  // not rounded: the five slabs are 16-byte multiples already
  CpeGrads cpe;
  SelfGrads self;
  FfnGrads ffn1;
  CrossKvGrads cross;
  FfnGrads ffn2;
  size_t end;
  PairGrads(float* slab, int C, int H, int Hd, Fields* rec = nullptr)
      : cpe(slab, 0, C, rec), self(slab, cpe.end, C, H, rec), ffn1(slab, self.end, C, Hd, rec), cross(slab, ffn1.end, C, H, rec),
        ffn2(slab, cross.end, C, Hd, rec), end(ffn2.end) {}
};
struct PairTmp {  // the five tmp regions, then d x4 | d x3 | d x2 | d x1: the gradients passed between the sub-blocks
  CpeTmp cpe;
  SelfTmp self;
  FfnTmp ffn1;
  CrossKvTmp cross;
  FfnTmp ffn2;
  PairActs d;   // d.x[0] = d x4, ... d.x[3] = d x1
  size_t end;
  PairTmp(float* slab, int M, int C, int Hd, int n_extra, int L, int G)
      : cpe(slab, 0, M, C), self(slab, al64(cpe.end), M, C, n_extra), ffn1(slab, al64(self.end), M, C, Hd),
        cross(slab, al64(ffn1.end), M, C, L, G), ffn2(slab, al64(cross.end), M, C, Hd), d(slab, al64(ffn2.end), M, C), end(d.end) {}
};

static inline size_t max3(size_t a, size_t b, size_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------------------------
// MLP sub-block
size_t lotus_ffn_saved_floats(int M, int C, int Hd) { return FfnSaved(nullptr, 0, M, C, Hd).end; }
size_t lotus_ffn_grads_floats(int C, int Hd) { return FfnGrads(nullptr, 0, C, Hd).end; }
size_t lotus_ffn_tmp_floats(int M, int C, int Hd) { return FfnTmp(nullptr, 0, M, C, Hd).end; }
size_t lotus_ffn_ws_main_bytes(int M, int C, int Hd) { return max3(lotus_linear_workspace(M, Hd, C), lotus_linear_workspace(M, C, Hd), 0); }
size_t lotus_ffn_ws_side_bytes(int M, int C, int Hd) {
  return max3(lotus_linear_wgrad_workspace(M, Hd, C), lotus_linear_wgrad_workspace(M, C, Hd), 0);
}

int lotus_ffn_fwd(const act_t* x, const float* g, const float* b, const float* w1, const float* b1, const float* w2,
                  const float* b2, act_t* y, float* saved, int M, int C, int Hd, float drop_p, unsigned long long seed1,
                  unsigned long long seed2, int precision, void* ws, size_t ws_bytes, void* counters, void* stream) {
  const FfnSaved sv(saved, 0, M, C, Hd);
  const Ws w = small_rows_only(Ws{ws, ws_bytes, counters}, M);
  CHECK(lotus_layernorm_fwd(x, nullptr, g, b, sv.n, sv.mean, sv.rstd, M, C, 1e-5f, stream));
  CHECK(lotus_linear_fwd(sv.n, w1, b1, nullptr, sv.a, sv.hpre, M, Hd, C, LOTUS_ACT_GELU, drop_p, seed1, precision, w.p, w.bytes, w.counters,
                         stream));
  return lotus_linear_fwd(sv.a, w2, b2, x, y, nullptr, M, C, Hd, LOTUS_ACT_NONE, drop_p, seed2, precision, w.p, w.bytes, w.counters, stream);
}

// dz_in (optional): dy already multiplied by the fc2 dropout mask (handed over by the next sub-block's backward).
// dz_out (optional, with dz_out_p > 0): dx times the dropout mask (dz_out_p, dz_out_seed) of the PREVIOUS sub-block.
int lotus_ffn_bwd(const act_t* dy, const act_t* dz_in, const act_t* x, const float* g, const float* w1, const float* w2,
                  const float* saved, act_t* dx, act_t* dz_out, float dz_out_p, unsigned long long dz_out_seed, float* grads,
                  float* tmp, int M, int C, int Hd, float drop_p, unsigned long long seed1, unsigned long long seed2,
                  int precision, void* ws_main, size_t ws_main_bytes, void* ws_side, size_t ws_side_bytes, void* counters_main,
                  void* counters_side, unsigned long long link, int join, void* stream, void* side) {
  const FfnSaved sv(saved, 0, M, C, Hd);
  const FfnGrads gr(grads, 0, C, Hd);
  const FfnTmp tp(tmp, 0, M, C, Hd);
  const Ws main{ws_main, ws_main_bytes, counters_main};
  const WgradLane wg(side, Ws{ws_side, ws_side_bytes, counters_side}, stream, main);
  const Ws w = small_rows_only(main, M);
  const act_t* dz;
  CHECK(masked_dy(dy, dz_in, tp.dz, (long)M * C, drop_p, seed2, link, stream, side, &dz));
  CHECK(lotus_linear_wgrad(dz, sv.a, gr.dw2, gr.db2, M, C, Hd, 0, precision, wg.ws.p, wg.ws.bytes, wg.ws.counters, wg.stream));
  PRODUCE_THEN_FORK(lotus_linear_dgrad(dz, w2, tp.dh, sv.hpre, nullptr, M, C, Hd, LOTUS_ACT_GELU, drop_p, seed1, precision, w.p, w.bytes,
                                       w.counters, stream));
  CHECK(lotus_linear_wgrad(tp.dh, sv.n, gr.dw1, gr.db1, M, Hd, C, 0, precision, wg.ws.p, wg.ws.bytes, wg.ws.counters, wg.stream));
  CHECK(dgrad_ln(tp.dh, w1, tp.dn, x, sv.mean, sv.rstd, g, dy, dx, dz_out, dz_out_p, dz_out_seed, gr.dg, gr.db, M, Hd, C, precision, w, tp.lnp,
                 tp.lnp_bytes, link, stream, side));
  if (side && join) CHECK(lotus_streamlink_wait(link, side, stream));
  return LOTUS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Patch self-attention sub-block
size_t lotus_selfattn_saved_floats(int M, int C, int H, int npad) { return SelfSaved(nullptr, 0, M, C, H, npad).end; }
size_t lotus_selfattn_grads_floats(int C, int H) { return SelfGrads(nullptr, 0, C, H).end; }
size_t lotus_selfattn_tmp_floats(int M, int C, int n_extra) { return SelfTmp(nullptr, 0, M, C, n_extra).end; }
size_t lotus_selfattn_ws_main_bytes(int M, int C, int H, int nblocks) {
  return max3(lotus_linear_workspace(M, 3 * C, C), lotus_linear_workspace(M, C, C), lotus_attention_bwd_workspace(nblocks, H));
}
size_t lotus_selfattn_ws_side_bytes(int M, int C) {
  return max3(lotus_linear_wgrad_workspace(M, 3 * C, C), lotus_linear_wgrad_workspace(M, C, C), 0);
}

int lotus_selfattn_fwd(const act_t* x, const float* g, const float* b, const float* wqkv, const float* bqkv, const float* qnw,
                       const float* qnb, const float* knw, const float* knb, const float* wp, const float* bp, act_t* y,
                       float* saved, const int* gidx, const int* owner, const int* tiles, int ntiles, int npad, int M, int C,
                       int H, float scale, float drop_p, unsigned long long seed, float attn_p, unsigned long long attn_seed,
                       int precision, void* ws, size_t ws_bytes, void* counters, void* stream) {
  const int d = C / H;
  const SelfSaved sv(saved, 0, M, C, H, npad);
  const Ws w = small_rows_only(Ws{ws, ws_bytes, counters}, M);
  CHECK(lotus_layernorm_fwd(x, nullptr, g, b, sv.n, sv.mean, sv.rstd, M, C, 1e-5f, stream));
  CHECK(lotus_linear_fwd(sv.n, wqkv, bqkv, nullptr, sv.qkv, nullptr, M, 3 * C, C, LOTUS_ACT_NONE, 0.f, 0, precision, w.p, w.bytes, w.counters,
                         stream));
  CHECK(lotus_attention_fwd(sv.qkv, 3L * C, 0, sv.qkv, 3L * C, C, 2 * C, gidx, gidx, owner, tiles, ntiles, qnw, qnb, knw, knb, sv.att, (long)C,
                            sv.lse, H, d, scale, 1e-6f, attn_p, attn_seed, noshadow(precision), 0, stream));
  return lotus_linear_fwd(sv.att, wp, bp, x, y, nullptr, M, C, C, LOTUS_ACT_NONE, drop_p, seed, precision, w.p, w.bytes, w.counters, stream);
}

int lotus_selfattn_bwd(const act_t* dy, const act_t* dz_in, const act_t* x, const float* g, const float* wqkv, const float* qnw,
                       const float* qnb, const float* knw, const float* knb, const float* wp, const float* saved, act_t* dx,
                       float* grads, float* tmp, const int* gidx, const int* owner, const int* tiles, const int* blocks, int nblocks,
                       const int* kext, const int* ext_pos, int n_extra, int npad, int M, int C, int H, float scale, float drop_p,
                       unsigned long long seed, float attn_p, unsigned long long attn_seed, int precision, void* ws_main,
                       size_t ws_main_bytes, void* ws_side, size_t ws_side_bytes, void* counters_main, void* counters_side,
                       unsigned long long link, int join, void* stream, void* side) {
  const int d = C / H;
  const SelfSaved sv(saved, 0, M, C, H, npad);
  const SelfGrads gr(grads, 0, C, H);
  const SelfTmp tp(tmp, 0, M, C, n_extra);
  const Ws main{ws_main, ws_main_bytes, counters_main};
  const WgradLane wg(side, Ws{ws_side, ws_side_bytes, counters_side}, stream, main);
  const Ws w = small_rows_only(main, M);
  const act_t* dz;
  CHECK(masked_dy(dy, dz_in, tp.dz, (long)M * C, drop_p, seed, link, stream, side, &dz));
  CHECK(lotus_linear_wgrad(dz, sv.att, gr.dwp, gr.dbp, M, C, C, 0, precision, wg.ws.p, wg.ws.bytes, wg.ws.counters, wg.stream));
  CHECK(lotus_linear_dgrad(dz, wp, tp.datt, nullptr, nullptr, M, C, C, LOTUS_ACT_NONE, 0.f, 0, precision, w.p, w.bytes, w.counters, stream));
  PRODUCE_THEN_FORK(lotus_attention_bwd(sv.qkv, 3L * C, 0, sv.qkv, 3L * C, C, 2 * C, gidx, gidx, owner, tiles, blocks, nblocks, qnw, qnb, knw, knb,
                                        sv.att, tp.datt, (long)C, sv.lse, tp.dqkv, 3L * C, 0, tp.dqkv, 3L * C, C, 2 * C, 0, 0, kext, ext_pos,
                                        n_extra, tp.extra, gr.gq, gr.bq, gr.gk, gr.bk, 0, H, d, scale, 1e-6f, attn_p, attn_seed,
                                        noshadow(precision), 0, ws_main, ws_main_bytes, stream));
  CHECK(lotus_linear_wgrad(tp.dqkv, sv.n, gr.dwqkv, gr.dbqkv, M, 3 * C, C, 0, precision, wg.ws.p, wg.ws.bytes, wg.ws.counters, wg.stream));
  CHECK(dgrad_ln(tp.dqkv, wqkv, tp.dn, x, sv.mean, sv.rstd, g, dy, dx, nullptr, 0.f, 0, gr.dg, gr.db, M, 3 * C, C, precision, w, tp.lnp,
                 tp.lnp_bytes, link, stream, side));
  if (side && join) CHECK(lotus_streamlink_wait(link, side, stream));
  return LOTUS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Cross-attention sub-block
size_t lotus_crossattn_saved_floats(int M, int C, int H, int L) { return CrossSaved(nullptr, 0, M, C, H, L).end; }
size_t lotus_crossattn_grads_floats(int C, int H, int Cc) { return CrossGrads(nullptr, 0, C, H, Cc).end; }
size_t lotus_crossattn_tmp_floats(int M, int C, int L, int G) { return CrossTmp(nullptr, 0, M, C, L, G).end; }
size_t lotus_crossattn_ws_main_bytes(int M, int C, int H, int L, int Cc, int nblocks) {
  return max3(lotus_linear_workspace(M, C, C), lotus_linear_workspace(L, 2 * C, Cc), lotus_attention_bwd_workspace(nblocks, H));
}
size_t lotus_crossattn_ws_side_bytes(int M, int C, int L, int Cc) {
  return max3(lotus_linear_wgrad_workspace(M, C, C), lotus_linear_wgrad_workspace(L, 2 * C, Cc), 0);
}

int lotus_crossattn_fwd(const act_t* x, const act_t* context, const float* g, const float* b, const float* wq, const float* bq,
                        const float* wkv, const float* bkv, const float* qnw, const float* qnb, const float* knw, const float* knb,
                        const float* wp, const float* bp, act_t* y, float* saved, const int* tiles, int ntiles, int M, int C, int H,
                        int L, int Cc, float scale, float drop_p, unsigned long long seed, float attn_p, unsigned long long attn_seed,
                        int precision, int k_max, void* ws, size_t ws_bytes, void* counters, void* stream) {
  const int d = C / H;
  const CrossSaved sv(saved, 0, M, C, H, L);
  const Ws w = small_rows_only(Ws{ws, ws_bytes, counters}, M), wL = small_rows_only(Ws{ws, ws_bytes, counters}, L);
  CHECK(lotus_layernorm_fwd(x, nullptr, g, b, sv.n, sv.mean, sv.rstd, M, C, 1e-5f, stream));
  CHECK(lotus_linear_fwd(sv.n, wq, bq, nullptr, sv.q, nullptr, M, C, C, LOTUS_ACT_NONE, 0.f, 0, precision, w.p, w.bytes, w.counters, stream));
  CHECK(lotus_linear_fwd(context, wkv, bkv, nullptr, sv.kv, nullptr, L, 2 * C, Cc, LOTUS_ACT_NONE, 0.f, 0, precision, wL.p, wL.bytes, wL.counters,
                         stream));
  CHECK(lotus_attention_fwd(sv.q, (long)C, 0, sv.kv, 2L * C, 0, C, nullptr, nullptr, nullptr, tiles, ntiles, qnw, qnb, knw, knb, sv.att, (long)C,
                            sv.lse, H, d, scale, 1e-6f, attn_p, attn_seed, noshadow(precision), k_max, stream));
  return lotus_linear_fwd(sv.att, wp, bp, x, y, nullptr, M, C, C, LOTUS_ACT_NONE, drop_p, seed, precision, w.p, w.bytes, w.counters, stream);
}

// dctx (optional): gradient of the context [L][Cc].  G = key-side partial slots of the attention backward.
int lotus_crossattn_bwd(const act_t* dy, const act_t* dz_in, const act_t* x, const act_t* context, const float* g, const float* wq,
                        const float* wkv, const float* qnw, const float* qnb, const float* knw, const float* knb, const float* wp,
                        const float* saved, act_t* dx, act_t* dctx, act_t* dz_out, float dz_out_p, unsigned long long dz_out_seed,
                        float* grads, float* tmp, const int* tiles, const int* blocks, int nblocks, int G, int M, int C, int H, int L,
                        int Cc, float scale, float drop_p, unsigned long long seed, float attn_p, unsigned long long attn_seed,
                        int precision, int k_max, void* ws_main, size_t ws_main_bytes, void* ws_side, size_t ws_side_bytes, void* counters_main,
                        void* counters_side, unsigned long long link, int join, void* stream, void* side) {
  const int d = C / H;
  const CrossSaved sv(saved, 0, M, C, H, L);
  const CrossGrads gr(grads, 0, C, H, Cc);
  const CrossTmp tp(tmp, 0, M, C, L, G);
  const Ws main{ws_main, ws_main_bytes, counters_main};
  const WgradLane wg(side, Ws{ws_side, ws_side_bytes, counters_side}, stream, main);
  const Ws w = small_rows_only(main, M), wL = small_rows_only(main, L);
  const act_t* dz;
  CHECK(masked_dy(dy, dz_in, tp.dz, (long)M * C, drop_p, seed, link, stream, side, &dz));
  CHECK(lotus_linear_wgrad(dz, sv.att, gr.dwp, gr.dbp, M, C, C, 0, precision, wg.ws.p, wg.ws.bytes, wg.ws.counters, wg.stream));
  CHECK(lotus_linear_dgrad(dz, wp, tp.datt, nullptr, nullptr, M, C, C, LOTUS_ACT_NONE, 0.f, 0, precision, w.p, w.bytes, w.counters, stream));
  const act_t* dkv_f = tp.dkv_part;
  {
    ForkAfter fa(link, side);  // dq and d kv: the last launch in here carries the fork event
    if (G > 1) lotus_tls_stop_event = nullptr;
    CHECK(lotus_attention_bwd(sv.q, (long)C, 0, sv.kv, 2L * C, 0, C, nullptr, nullptr, nullptr, tiles, blocks, nblocks, qnw, qnb, knw, knb, sv.att,
                              tp.datt, (long)C, sv.lse, tp.dq, (long)C, 0, tp.dkv_part, 2L * C, 0, C, (long)L * 2 * C, 0, nullptr, nullptr, 0,
                              nullptr, gr.gq, gr.bq, gr.gk, gr.bk, 0, H, d, scale, 1e-6f, attn_p, attn_seed, noshadow(precision), k_max, ws_main,
                              ws_main_bytes, stream));
    if (G > 1) {  // fixed-order sum of the key-side partial slots
      lotus_tls_stop_event = fa.ev;
      CHECK(lotus_sum_slabs(tp.dkv_part, tp.dkv, (long)L * 2 * C, (long)L * 2 * C, G, stream));
      dkv_f = tp.dkv;
    }
    CHECK(fa.wait());
  }
  CHECK(lotus_linear_wgrad(dkv_f, context, gr.dwkv, gr.dbkv, L, 2 * C, Cc, 0, precision, wg.ws.p, wg.ws.bytes, wg.ws.counters, wg.stream));
  CHECK(lotus_linear_wgrad(tp.dq, sv.n, gr.dwq, gr.dbq, M, C, C, 0, precision, wg.ws.p, wg.ws.bytes, wg.ws.counters, wg.stream));
  if (dctx)
    CHECK(lotus_linear_dgrad(dkv_f, wkv, dctx, nullptr, nullptr, L, 2 * C, Cc, LOTUS_ACT_NONE, 0.f, 0, precision, wL.p, wL.bytes, wL.counters,
                             stream));
  CHECK(dgrad_ln(tp.dq, wq, tp.dn, x, sv.mean, sv.rstd, g, dy, dx, dz_out, dz_out_p, dz_out_seed, gr.dg, gr.db, M, C, C, precision, w, tp.lnp,
                 tp.lnp_bytes, link, stream, side));
  if (side && join) CHECK(lotus_streamlink_wait(link, side, stream));
  return LOTUS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Cross-attention sub-block with PRECOMPUTED keys / values.  The context is the same for every CABlock of a forward pass
// (model_ca.py:46-67: kv = Linear(256 -> 2C)(context)), so the model projects it once for all blocks — one product
// [L, 256] x [256, sum 2C] — and each block reads its column slice `kv` (row stride kv_ld) of that slab; backward writes
// d kv into the block's slice `dkv` (row stride dkv_ld) of the shared gradient slab, from which ONE input-gradient and ONE
// weight-gradient product follow (ops.KvAllFn).  Everything else is lotus_crossattn_fwd / _bwd.
size_t lotus_crossattn_kv_saved_floats(int M, int C, int H) { return CrossKvSaved(nullptr, 0, M, C, H).end; }
size_t lotus_crossattn_kv_grads_floats(int C, int H) { return CrossKvGrads(nullptr, 0, C, H).end; }
size_t lotus_crossattn_kv_tmp_floats(int M, int C, int L, int G) { return CrossKvTmp(nullptr, 0, M, C, L, G).end; }
size_t lotus_crossattn_kv_ws_main_bytes(int M, int C, int H, int nblocks) {
  return max3(lotus_linear_workspace(M, C, C), lotus_attention_bwd_workspace(nblocks, H), 0);
}
size_t lotus_crossattn_kv_ws_side_bytes(int M, int C) { return lotus_linear_wgrad_workspace(M, C, C); }

int lotus_crossattn_kv_fwd(const act_t* x, const act_t* kv, long kv_ld, const float* g, const float* b, const float* wq, const float* bq,
                           const float* qnw, const float* qnb, const float* knw, const float* knb, const float* wp, const float* bp,
                           act_t* y, float* saved, const int* tiles, int ntiles, int M, int C, int H, float scale, float drop_p,
                           unsigned long long seed, float attn_p, unsigned long long attn_seed, int precision, int k_max, void* ws,
                           size_t ws_bytes, void* counters, void* stream) {
  const int d = C / H;
  const CrossKvSaved sv(saved, 0, M, C, H);
  const Ws w = small_rows_only(Ws{ws, ws_bytes, counters}, M);
  CHECK(lotus_layernorm_fwd(x, nullptr, g, b, sv.n, sv.mean, sv.rstd, M, C, 1e-5f, stream));
  CHECK(lotus_linear_fwd(sv.n, wq, bq, nullptr, sv.q, nullptr, M, C, C, LOTUS_ACT_NONE, 0.f, 0, precision, w.p, w.bytes, w.counters, stream));
  CHECK(lotus_attention_fwd(sv.q, (long)C, 0, kv, kv_ld, 0, C, nullptr, nullptr, nullptr, tiles, ntiles, qnw, qnb, knw, knb, sv.att, (long)C,
                            sv.lse, H, d, scale, 1e-6f, attn_p, attn_seed, noshadow(precision), k_max, stream));
  return lotus_linear_fwd(sv.att, wp, bp, x, y, nullptr, M, C, C, LOTUS_ACT_NONE, drop_p, seed, precision, w.p, w.bytes, w.counters, stream);
}

int lotus_crossattn_kv_bwd(const act_t* dy, const act_t* dz_in, const act_t* x, const act_t* kv, long kv_ld, const float* g,
                           const float* wq, const float* qnw, const float* qnb, const float* knw, const float* knb, const float* wp,
                           const float* saved, act_t* dx, act_t* dkv, long dkv_ld, act_t* dz_out, float dz_out_p,
                           unsigned long long dz_out_seed, float* grads, float* tmp, const int* tiles, const int* blocks, int nblocks,
                           int G, int M, int C, int H, int L, float scale, float drop_p, unsigned long long seed, float attn_p,
                           unsigned long long attn_seed, int precision, int k_max, void* ws_main, size_t ws_main_bytes, void* ws_side,
                           size_t ws_side_bytes, void* counters_main, void* counters_side, unsigned long long link, int join,
                           void* stream, void* side) {
  const int d = C / H;
  const CrossKvSaved sv(saved, 0, M, C, H);
  const CrossKvGrads gr(grads, 0, C, H);
  const CrossKvTmp tp(tmp, 0, M, C, L, G);
  const Ws main{ws_main, ws_main_bytes, counters_main};
  const WgradLane wg(side, Ws{ws_side, ws_side_bytes, counters_side}, stream, main);
  const Ws w = small_rows_only(main, M);
  const act_t* dz;
  CHECK(masked_dy(dy, dz_in, tp.dz, (long)M * C, drop_p, seed, link, stream, side, &dz));
  CHECK(lotus_linear_wgrad(dz, sv.att, gr.dwp, gr.dbp, M, C, C, 0, precision, wg.ws.p, wg.ws.bytes, wg.ws.counters, wg.stream));
  CHECK(lotus_linear_dgrad(dz, wp, tp.datt, nullptr, nullptr, M, C, C, LOTUS_ACT_NONE, 0.f, 0, precision, w.p, w.bytes, w.counters, stream));
  // d q (-> the weight gradient of the q projection on the side stream) and d kv: with one key-side slot the attention
  // backward writes the block's slice of the shared gradient slab directly, else the slots are summed into it
  PRODUCE_THEN_FORK(lotus_attention_bwd(sv.q, (long)C, 0, kv, kv_ld, 0, C, nullptr, nullptr, nullptr, tiles, blocks, nblocks, qnw, qnb, knw, knb,
                                        sv.att, tp.datt, (long)C, sv.lse, tp.dq, (long)C, 0, G > 1 ? tp.dkv_part : dkv, G > 1 ? 2L * C : dkv_ld, 0,
                                        C, G > 1 ? (long)L * 2 * C : 0, 0, nullptr, nullptr, 0, nullptr, gr.gq, gr.bq, gr.gk, gr.bk, 0, H, d, scale,
                                        1e-6f, attn_p, attn_seed, noshadow(precision), k_max, ws_main, ws_main_bytes, stream));
  if (G > 1) CHECK(lotus_sum_slabs_ld(tp.dkv_part, dkv, L, 2 * C, dkv_ld, (long)L * 2 * C, G, stream));
  CHECK(lotus_linear_wgrad(tp.dq, sv.n, gr.dwq, gr.dbq, M, C, C, 0, precision, wg.ws.p, wg.ws.bytes, wg.ws.counters, wg.stream));
  CHECK(dgrad_ln(tp.dq, wq, tp.dn, x, sv.mean, sv.rstd, g, dy, dx, dz_out, dz_out_p, dz_out_seed, gr.dg, gr.db, M, C, C, precision, w, tp.lnp,
                 tp.lnp_bytes, link, stream, side));
  if (side && join) CHECK(lotus_streamlink_wait(link, side, stream));
  return LOTUS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Conditional positional encoding; xs == x in the encoder, the stale skip branch in the decoder (SURVEY.md Trap 3).
size_t lotus_cpe_saved_floats(int n, int C) { return CpeSaved(nullptr, 0, n, C).end; }
size_t lotus_cpe_grads_floats(int C) { return CpeGrads(nullptr, 0, C).end; }
size_t lotus_cpe_tmp_floats(int n, int C) { return CpeTmp(nullptr, 0, n, C).end; }
size_t lotus_cpe_ws_main_bytes(int n, int C) { return lotus_linear_workspace(n, C, C); }
size_t lotus_cpe_ws_conv_bytes(int n, int C) { return lotus_subm_conv_workspace(n, C, C); }
size_t lotus_cpe_ws_side_bytes(int n, int C) {
  return max3(lotus_linear_wgrad_workspace(n, C, C), lotus_subm_conv_wgrad_workspace(n, 27, C, C), 0);
}

int lotus_cpe_fwd(const act_t* x, const act_t* xs, const float* cw, const float* cw_packed, const float* cb, const float* lw,
                  const float* lb, const float* g, const float* b, act_t* y, float* saved, const int* nbr27, const int* order0,
                  const int* tap_plan, int n, int C, int precision, void* ws, size_t ws_bytes, void* ws_conv, size_t ws_conv_bytes, void* counters, void* stream) {
  const CpeSaved sv(saved, 0, n, C);
  const Ws w = small_rows_only(Ws{ws, ws_bytes, counters}, n);
  CHECK(lotus_subm_conv(0, xs, cw, cw_packed, cb, nullptr, sv.c, nbr27, order0, n, 27, C, C, noshadow(precision), tap_plan, ws_conv, ws_conv_bytes, stream));
  CHECK(lotus_linear_fwd(sv.c, lw, lb, nullptr, sv.l, nullptr, n, C, C, LOTUS_ACT_NONE, 0.f, 0, precision, w.p, w.bytes, w.counters, stream));
  return lotus_layernorm_fwd(sv.l, x, g, b, y, sv.mean, sv.rstd, n, C, 1e-5f, stream);
}

// dx_conv = input gradient of the convolution (+ dy when add_dy: the encoder case, where it IS d x).  n_dup != 0: the
// level holds several points per voxel (code0 / order0 of the level drive the fold, nbr27[13] the mask).
int lotus_cpe_bwd(const act_t* dy, const act_t* xs, const float* cw, const float* cw_packed, const float* lw, const float* g,
                  const float* saved, act_t* dx_conv, int add_dy, float* grads, float* tmp, const int* nbr27, const int* order0,
                  const int* tap_plan, const long long* code0, int n_dup, int n, int C, int precision, void* ws_main, size_t ws_main_bytes, void* ws_conv,
                  size_t ws_conv_bytes, void* ws_side, size_t ws_side_bytes, void* counters_main, void* counters_side,
                  unsigned long long link, int join, void* stream, void* side) {
  const CpeSaved sv(saved, 0, n, C);
  const CpeGrads gr(grads, 0, C);
  const CpeTmp tp(tmp, 0, n, C);
  const Ws main{ws_main, ws_main_bytes, counters_main};
  const WgradLane wg(side, Ws{ws_side, ws_side_bytes, counters_side}, stream, main);
  const Ws w = small_rows_only(main, n);
  if (side) {
    PRODUCE_THEN_FORK(lotus_layernorm_bwd(dy, sv.l, sv.mean, sv.rstd, g, nullptr, tp.dl, nullptr, nullptr, n, C, 0, nullptr, 0.f, 0, tp.lnp,
                                          tp.lnp_bytes, stream));
    CHECK(lotus_layernorm_bwd_params(tp.lnp, n, C, gr.dg, gr.db, 0, side));
  } else {
    CHECK(lotus_layernorm_bwd(dy, sv.l, sv.mean, sv.rstd, g, nullptr, tp.dl, gr.dg, gr.db, n, C, 0, nullptr, 0.f, 0, tp.lnp, tp.lnp_bytes, stream));
  }
  CHECK(lotus_linear_wgrad(tp.dl, sv.c, gr.dlw, gr.dlb, n, C, C, 0, precision, wg.ws.p, wg.ws.bytes, wg.ws.counters, wg.stream));
  PRODUCE_THEN_FORK(lotus_linear_dgrad(tp.dl, lw, tp.dc, nullptr, nullptr, n, C, C, LOTUS_ACT_NONE, 0.f, 0, precision, w.p, w.bytes, w.counters,
                                       stream));
  CHECK(lotus_subm_conv_wgrad(tp.dc, xs, gr.dcw, gr.dcb, nbr27, n, 27, C, C, 0, noshadow(precision), wg.ws.p, wg.ws.bytes, wg.stream));
  const act_t* dsrc = tp.dc;
  if (n_dup != 0) {
    CHECK(lotus_conv_dup_fold(tp.dc, code0, order0, n, C, tp.dyr, stream));
    dsrc = tp.dyr;
  }
  CHECK(lotus_subm_conv(1, dsrc, cw, cw_packed, nullptr, add_dy ? dy : nullptr, dx_conv, nbr27, order0, n, 27, C, C, noshadow(precision), tap_plan, ws_conv,
                        ws_conv_bytes, stream));
  if (n_dup != 0) CHECK(lotus_conv_dup_mask(dx_conv, add_dy ? dy : nullptr, nbr27 + (size_t)13 * n, n, C, stream));
  if (side && join) CHECK(lotus_streamlink_wait(link, side, stream));
  return LOTUS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// One (Block, CABlock) pair per call (round 4): the five sub-blocks above chained on the host side of the C-ABI —
//   x1 = cpe(x, xs);  x2 = selfattn(x1);  x3 = ffn(x2);  x4 = crossattn_kv(x3, kv);  y = ffn(x4)
// (model_ca.py:270-310: Block i then CABlock i of a stage) — with the backward-pass hand-overs of the pre-masked
// gradients (ops.Handoff) wired inside.  Exactly the launches of the five composite calls in the same order on the same
// streams, so results are bit-identical to issuing them one by one (tests/test_gpu_round4.py); what it saves is host time:
// one Python -> C transition, one autograd node and one set of allocations per direction instead of five.
// Arguments travel as three host arrays: device pointers P, integers I, floating-point scalars F.  The lists below ARE the
// index tables: the enums are generated from them, and lotus_pair_ptr_names / lotus_pair_int_names hand the same lists to
// the caller as strings (ops._pair_tables builds its name -> index dicts from those; tests/test_composite_layout.py).
#define PAIR_PTRS(_)                                                                                                         \
  _(X) _(XS) _(KV) _(Y) _(ACTS) _(SAVED) _(CW) _(CWP) _(CB) _(LW) _(LB) _(G0) _(B0)                     /* cpe */             \
  _(G1) _(B1) _(WQKV) _(BQKV) _(QNW) _(QNB) _(KNW) _(KNB) _(WP) _(BP)                                   /* self-attention */  \
  _(G2) _(B2) _(W1) _(B1F) _(W2) _(B2F)                                                                 /* mlp of the Block */ \
  _(G3) _(B3) _(WQ) _(BQ) _(CQNW) _(CQNB) _(CKNW) _(CKNB) _(CWP2) _(CBP2)                               /* cross-attention */ \
  _(G4) _(B4) _(W3) _(B3F) _(W4) _(B4F)                                                                 /* mlp of the CABlock */ \
  _(NBR27) _(ORDER0) _(TAPPLAN) _(CODE0) _(GIDX) _(OWNER) _(STILES) _(SBLOCKS) _(KEXT) _(EXTPOS) _(CATILES) _(CABLOCKS)       \
  _(WS_MAIN) _(WS_SIDE) _(WS_CONV) _(CNT_MAIN) _(CNT_SIDE) _(STREAM) _(SIDE)                                                   \
  _(DY) _(DX) _(DXS) _(DKV) _(GRADS) _(TMP)                                                             /* backward only */
#define PAIR_INTS(_)                                                                                                         \
  _(M) _(C) _(H) _(HD) _(NPAD) _(NSTILES) _(NEXTRA) _(L) _(NCATILES) _(NCABLOCKS) _(G) _(KMAX) _(NDUP) _(SAME) _(PREC) _(KV_LD) \
  _(DKV_LD) _(WS_MAIN) _(WS_SIDE) _(WS_CONV) _(LINK) _(SEED_SELF) _(SEED_FFN1) _(SEED_CROSS) _(SEED_FFN2)
#define PP_ENUM(name) PP_##name,
#define PI_ENUM(name) PI_##name,
#define NAME_STR(name) #name " "
enum PairPtr { PAIR_PTRS(PP_ENUM) PP_COUNT };
enum PairInt { PAIR_INTS(PI_ENUM) PI_COUNT };
enum PairFlt { PF_DROP, PF_ATTN, PF_SCALE, PF_COUNT };
#ifndef LOTUS_ACT_BF16  // (the names are the same in both builds: defined once, in the fp32 one)
const char* lotus_pair_ptr_names(void) { return PAIR_PTRS(NAME_STR); }
const char* lotus_pair_int_names(void) { return PAIR_INTS(NAME_STR); }
#endif
int lotus_pair_nptr(void) { return PP_COUNT; }
int lotus_pair_nint(void) { return PI_COUNT; }

static inline unsigned long long pair_mix(unsigned long long seed, unsigned long long k) {  // == ops.mix_seed (splitmix64 finaliser)
  unsigned long long z = seed + 0x9E3779B97F4A7C15ULL * (k + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

size_t lotus_pair_acts_floats(int M, int C) { return PairActs(nullptr, 0, M, C).end; }
size_t lotus_pair_saved_floats(int M, int C, int H, int Hd, int npad) { return PairSaved(nullptr, M, C, H, Hd, npad).end; }
size_t lotus_pair_grads_floats(int C, int H, int Hd) { return PairGrads(nullptr, C, H, Hd).end; }
size_t lotus_pair_tmp_floats(int M, int C, int Hd, int n_extra, int L, int G) { return PairTmp(nullptr, M, C, Hd, n_extra, L, G).end; }
size_t lotus_pair_ws_main_bytes(int M, int C, int H, int Hd, int nblocks_self, int nblocks_ca) {
  return max3(max3(lotus_cpe_ws_main_bytes(M, C), lotus_selfattn_ws_main_bytes(M, C, H, nblocks_self), lotus_ffn_ws_main_bytes(M, C, Hd)),
              lotus_crossattn_kv_ws_main_bytes(M, C, H, nblocks_ca), 0);
}
size_t lotus_pair_ws_side_bytes(int M, int C, int Hd) {
  return max3(max3(lotus_cpe_ws_side_bytes(M, C), lotus_selfattn_ws_side_bytes(M, C), lotus_ffn_ws_side_bytes(M, C, Hd)),
              lotus_crossattn_kv_ws_side_bytes(M, C), 0);
}
size_t lotus_pair_ws_conv_bytes(int M, int C) { return lotus_cpe_ws_conv_bytes(M, C); }

// Where each parameter gradient lies in the `grads` slab of a composite: fills (offset, length) in floats, in slab order,
// for the first `cap` fields and returns the number of fields (the pair: its five sub-blocks one after the other).
// kind: 0 ffn, 1 selfattn, 2 crossattn, 3 crossattn_kv, 4 cpe, 5 pair; dimensions a kind does not have are ignored.
int lotus_composite_grads_layout(int kind, int C, int H, int Hd, int Cc, long long* off, long long* len, int cap) {
  Fields rec{off, len, cap, 0};
  switch (kind) {
    case 0: FfnGrads(nullptr, 0, C, Hd, &rec); break;
    case 1: SelfGrads(nullptr, 0, C, H, &rec); break;
    case 2: CrossGrads(nullptr, 0, C, H, Cc, &rec); break;
    case 3: CrossKvGrads(nullptr, 0, C, H, &rec); break;
    case 4: CpeGrads(nullptr, 0, C, &rec); break;
    case 5: PairGrads(nullptr, C, H, Hd, &rec); break;
    default: lotus_set_error("lotus_composite_grads_layout: kind %d is none of 0..5", kind); return LOTUS_E_ARG;
  }
  return rec.n;
}

#define PPTR(T, i) ((T)P[i])
int lotus_pair_fwd(const void* const* P, const long long* I, const double* F) {
  const int M = (int)I[PI_M], C = (int)I[PI_C], H = (int)I[PI_H], Hd = (int)I[PI_HD], npad = (int)I[PI_NPAD];
  const int prec = (int)I[PI_PREC];
  const float drop = (float)F[PF_DROP], attn_p = (float)F[PF_ATTN], scale = (float)F[PF_SCALE];
  void* ws = PPTR(void*, PP_WS_MAIN);
  const size_t ws_b = (size_t)I[PI_WS_MAIN];
  void* cnt = PPTR(void*, PP_CNT_MAIN);
  void* st = PPTR(void*, PP_STREAM);
  const PairActs x(PPTR(const float*, PP_ACTS), 0, M, C);
  const PairSaved sv(PPTR(const float*, PP_SAVED), M, C, H, Hd, npad);
  const unsigned long long s_self = (unsigned long long)I[PI_SEED_SELF], s_f1 = (unsigned long long)I[PI_SEED_FFN1];
  const unsigned long long s_cross = (unsigned long long)I[PI_SEED_CROSS], s_f2 = (unsigned long long)I[PI_SEED_FFN2];
  CHECK(lotus_cpe_fwd(PPTR(const act_t*, PP_X), PPTR(const act_t*, PP_XS), PPTR(const float*, PP_CW), PPTR(const float*, PP_CWP),
                      PPTR(const float*, PP_CB), PPTR(const float*, PP_LW), PPTR(const float*, PP_LB), PPTR(const float*, PP_G0),
                      PPTR(const float*, PP_B0), x.x[0], sv.cpe.base, PPTR(const int*, PP_NBR27), PPTR(const int*, PP_ORDER0), PPTR(const int*, PP_TAPPLAN), M, C, prec, ws, ws_b,
                      PPTR(void*, PP_WS_CONV), (size_t)I[PI_WS_CONV], cnt, st));
  CHECK(lotus_selfattn_fwd(x.x[0], PPTR(const float*, PP_G1), PPTR(const float*, PP_B1), PPTR(const float*, PP_WQKV), PPTR(const float*, PP_BQKV),
                           PPTR(const float*, PP_QNW), PPTR(const float*, PP_QNB), PPTR(const float*, PP_KNW), PPTR(const float*, PP_KNB),
                           PPTR(const float*, PP_WP), PPTR(const float*, PP_BP), x.x[1], sv.self.base, PPTR(const int*, PP_GIDX),
                           PPTR(const int*, PP_OWNER), PPTR(const int*, PP_STILES), (int)I[PI_NSTILES], npad, M, C, H, scale, drop, s_self,
                           attn_p, pair_mix(s_self, 1), prec, ws, ws_b, cnt, st));
  CHECK(lotus_ffn_fwd(x.x[1], PPTR(const float*, PP_G2), PPTR(const float*, PP_B2), PPTR(const float*, PP_W1), PPTR(const float*, PP_B1F),
                      PPTR(const float*, PP_W2), PPTR(const float*, PP_B2F), x.x[2], sv.ffn1.base, M, C, Hd, drop, s_f1, pair_mix(s_f1, 1), prec, ws,
                      ws_b, cnt, st));
  CHECK(lotus_crossattn_kv_fwd(x.x[2], PPTR(const act_t*, PP_KV), (long)I[PI_KV_LD], PPTR(const float*, PP_G3), PPTR(const float*, PP_B3),
                               PPTR(const float*, PP_WQ), PPTR(const float*, PP_BQ), PPTR(const float*, PP_CQNW), PPTR(const float*, PP_CQNB),
                               PPTR(const float*, PP_CKNW), PPTR(const float*, PP_CKNB), PPTR(const float*, PP_CWP2),
                               PPTR(const float*, PP_CBP2), x.x[3], sv.cross.base, PPTR(const int*, PP_CATILES), (int)I[PI_NCATILES], M, C, H, scale,
                               drop, s_cross, attn_p, pair_mix(s_cross, 1), prec, (int)I[PI_KMAX], ws, ws_b, cnt, st));
  return lotus_ffn_fwd(x.x[3], PPTR(const float*, PP_G4), PPTR(const float*, PP_B4), PPTR(const float*, PP_W3), PPTR(const float*, PP_B3F),
                       PPTR(const float*, PP_W4), PPTR(const float*, PP_B4F), PPTR(act_t*, PP_Y), sv.ffn2.base, M, C, Hd, drop, s_f2,
                       pair_mix(s_f2, 1), prec, ws, ws_b, cnt, st);
}

// dxs = input gradient of the convolution (added into dx when xs is x: PI_SAME).
int lotus_pair_bwd(const void* const* P, const long long* I, const double* F) {
  const int M = (int)I[PI_M], C = (int)I[PI_C], H = (int)I[PI_H], Hd = (int)I[PI_HD], npad = (int)I[PI_NPAD];
  const int n_extra = (int)I[PI_NEXTRA], L = (int)I[PI_L], G = (int)I[PI_G], prec = (int)I[PI_PREC];
  const float drop = (float)F[PF_DROP], attn_p = (float)F[PF_ATTN], scale = (float)F[PF_SCALE];
  void* wm = PPTR(void*, PP_WS_MAIN);
  void* wsd = PPTR(void*, PP_WS_SIDE);
  const size_t wm_b = (size_t)I[PI_WS_MAIN], wsd_b = (size_t)I[PI_WS_SIDE];
  void* cm = PPTR(void*, PP_CNT_MAIN);
  void* cs = PPTR(void*, PP_CNT_SIDE);
  void* st = PPTR(void*, PP_STREAM);
  void* side = PPTR(void*, PP_SIDE);
  const unsigned long long link = (unsigned long long)I[PI_LINK];
  const PairActs x(PPTR(const float*, PP_ACTS), 0, M, C);
  const PairSaved sv(PPTR(const float*, PP_SAVED), M, C, H, Hd, npad);
  const PairGrads gr(PPTR(float*, PP_GRADS), C, H, Hd);
  const PairTmp tp(PPTR(float*, PP_TMP), M, C, Hd, n_extra, L, G);
  act_t *d4 = tp.d.x[0], *d3 = tp.d.x[1], *d2 = tp.d.x[2];  // d x4, d x3, d x2 are temporaries; d x1 = the gradient the cpe receives
  const unsigned long long s_self = (unsigned long long)I[PI_SEED_SELF], s_f1 = (unsigned long long)I[PI_SEED_FFN1];
  const unsigned long long s_cross = (unsigned long long)I[PI_SEED_CROSS], s_f2 = (unsigned long long)I[PI_SEED_FFN2];
  // the pre-masked gradient handed from a sub-block's LayerNorm backward to its predecessor lives in the predecessor's
  // tmp.dz (which the predecessor does not fill itself then): cross <- ffn2, ffn1 <- cross, self <- ffn1
  const bool hand = drop > 0.f;
  act_t* dz_cross = hand ? tp.cross.dz : nullptr;
  act_t* dz_ffn1 = hand ? tp.ffn1.dz : nullptr;
  act_t* dz_self = hand ? tp.self.dz : nullptr;
  const float hand_p = hand ? drop : 0.f;
  // d x1 (what the cpe backward receives).  Encoder (xs is x): a temporary, the cpe backward writes conv-gradient + d x1
  // to PP_DX.  Decoder (xs = the stale skip branch): d x1 IS the gradient of x (the residual passes it through) and the
  // convolution's input gradient goes to PP_DXS.
  const int same = (int)I[PI_SAME];
  act_t* d1 = same ? tp.d.x[3] : PPTR(act_t*, PP_DX);
  // mlp of the CABlock: dz_out masks d x4 with the cross-attention's projection dropout (drop, s_cross)
  CHECK(lotus_ffn_bwd(PPTR(const act_t*, PP_DY), nullptr, x.x[3], PPTR(const float*, PP_G4), PPTR(const float*, PP_W3), PPTR(const float*, PP_W4),
                      sv.ffn2.base, d4, dz_cross, hand_p, s_cross, gr.ffn2.base, tp.ffn2.base, M, C, Hd, drop, s_f2, pair_mix(s_f2, 1),
                      prec, wm, wm_b, wsd, wsd_b, cm, cs, link, 0, st, side));
  // cross-attention: dz_out masks d x3 with the fc2 dropout of the Block's mlp (drop, mix(s_f1, 1))
  CHECK(lotus_crossattn_kv_bwd(d4, dz_cross, x.x[2], PPTR(const act_t*, PP_KV), (long)I[PI_KV_LD], PPTR(const float*, PP_G3),
                               PPTR(const float*, PP_WQ), PPTR(const float*, PP_CQNW), PPTR(const float*, PP_CQNB), PPTR(const float*, PP_CKNW),
                               PPTR(const float*, PP_CKNB), PPTR(const float*, PP_CWP2), sv.cross.base, d3, PPTR(act_t*, PP_DKV), (long)I[PI_DKV_LD],
                               dz_ffn1, hand_p, pair_mix(s_f1, 1), gr.cross.base, tp.cross.base, PPTR(const int*, PP_CATILES),
                               PPTR(const int*, PP_CABLOCKS), (int)I[PI_NCABLOCKS], G, M, C, H, L, scale, drop, s_cross, attn_p,
                               pair_mix(s_cross, 1), prec, (int)I[PI_KMAX], wm, wm_b, wsd, wsd_b, cm, cs, link, 0, st, side));
  // mlp of the Block: dz_out masks d x2 with the self-attention's projection dropout (drop, s_self)
  CHECK(lotus_ffn_bwd(d3, dz_ffn1, x.x[1], PPTR(const float*, PP_G2), PPTR(const float*, PP_W1), PPTR(const float*, PP_W2), sv.ffn1.base,
                      d2, dz_self, hand_p, s_self, gr.ffn1.base, tp.ffn1.base, M, C, Hd, drop, s_f1, pair_mix(s_f1, 1), prec, wm,
                      wm_b, wsd, wsd_b, cm, cs, link, 0, st, side));
  CHECK(lotus_selfattn_bwd(d2, dz_self, x.x[0], PPTR(const float*, PP_G1), PPTR(const float*, PP_WQKV), PPTR(const float*, PP_QNW),
                           PPTR(const float*, PP_QNB), PPTR(const float*, PP_KNW), PPTR(const float*, PP_KNB), PPTR(const float*, PP_WP), sv.self.base,
                           d1, gr.self.base, tp.self.base, PPTR(const int*, PP_GIDX), PPTR(const int*, PP_OWNER), PPTR(const int*, PP_STILES),
                           PPTR(const int*, PP_SBLOCKS), (int)I[PI_NSTILES], PPTR(const int*, PP_KEXT), PPTR(const int*, PP_EXTPOS), n_extra, npad,
                           M, C, H, scale, drop, s_self, attn_p, pair_mix(s_self, 1), prec, wm, wm_b, wsd, wsd_b, cm, cs, link, 0, st, side));
  // cpe: d x = d x1 (+ the convolution's input gradient when xs is x); separate xs -> its gradient goes to dxs
  return lotus_cpe_bwd(d1, PPTR(const act_t*, PP_XS), PPTR(const float*, PP_CW), PPTR(const float*, PP_CWP), PPTR(const float*, PP_LW),
                       PPTR(const float*, PP_G0), sv.cpe.base, same ? PPTR(act_t*, PP_DX) : PPTR(act_t*, PP_DXS), same, gr.cpe.base, tp.cpe.base,
                       PPTR(const int*, PP_NBR27), PPTR(const int*, PP_ORDER0), PPTR(const int*, PP_TAPPLAN), PPTR(const long long*, PP_CODE0), (int)I[PI_NDUP], M, C, prec, wm,
                       wm_b, PPTR(void*, PP_WS_CONV), (size_t)I[PI_WS_CONV], wsd, wsd_b, cm, cs, link, 0, st, side);
}
#undef PPTR

}  // extern "C"
