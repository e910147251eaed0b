// lotus-hip: which kernel the calling thread's last attention launch was given to (attention.hip, attention_rpe.hip).  Written by
// lotus_attention_fwd / _bwd and lotus_attention_rpe_fwd / _bwd where the kernel is chosen and before the launch is attempted (so it is set on a machine without a
// device too); a call that launches nothing — an argument refusal, ntiles == 0, nblocks == 0 — leaves the record as it was.
// Library-internal like lotus_tls_conv_route (conv_route.h) and `__thread` for the same reason; lotus_attention_last_route
// copies it out.  Fields: include/lotus_hip.h.
#pragma once

#define LOTUS_ATTN_FWD 1    // attn_fwd_kernel<PREC, NORM>
#define LOTUS_ATTN_BWD 2    // attn_bwd_kernel<1 | 3>
#define LOTUS_ATTN_BWD2 3   // attn_bwd2_kernel<NORM>
#define LOTUS_ATTN_XQ 4     // xq_fwd_kernel<D> / xq_bwd_kernel<D>
#define LOTUS_ATTN_XQ2 5    // xq2_fwd_kernel<4> / xq2_bwd_kernel<4>
#define LOTUS_ATTN_RPE_FWD 6  // attn_rpe_fwd_kernel<NORM> (attention_rpe.hip: lotus_attention_rpe_fwd)
#define LOTUS_ATTN_RPE_BWD 7  // attn_rpe_bwd_kernel<NORM> (attention_rpe.hip: lotus_attention_rpe_bwd)
#define LOTUS_ATTN_LONG_FWD 8  // attn_long_fwd_kernel<NORM> (attention_long.hip: lotus_attention_long_fwd)
#define LOTUS_ATTN_LONG_BWD 9  // attn_long_dq_kernel<NORM> + attn_long_dkv_kernel<NORM> (attention_long.hip: lotus_attention_long_bwd)

#define LOTUS_ATTN_TAIL_FIXUP 1      // attn_extra_fixup_kernel follows the main kernel
#define LOTUS_ATTN_TAIL_LN_REDUCE 2  // attn_ln_reduce_kernel follows
#define LOTUS_ATTN_TAIL_RPE_MERGE 4  // attn_rpe_merge_kernel follows (the table gradient of family 7)

extern __attribute__((visibility("hidden"))) __thread int lotus_tls_attn_route[8];
static inline void lotus_note_attn_route(int family, int direction, int targ, int precision, int norm, int threads, int lds_bytes,
                                         int tail) {
  int* r = lotus_tls_attn_route;
  r[0] = family; r[1] = direction; r[2] = targ; r[3] = precision; r[4] = norm; r[5] = threads; r[6] = lds_bytes; r[7] = tail;
}
