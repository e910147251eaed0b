// lotus-hip: which kernel the calling thread's last sparse-convolution launch was given to (conv.hip, conv_pairs.hip).
// Written beside every launch of lotus_subm_conv / lotus_subm_conv_wgrad, where the kernel is chosen and before the launch is
// attempted (so it is set on a machine without a device too); a path that launches nothing — an argument refusal, n == 0 —
// leaves the record as it was.  Library-internal like lotus_tls_dense_route (gemm_common.h) and `__thread` for the same
// reason; lotus_conv_last_route copies it out.  Fields: include/lotus_hip.h.
#pragma once

#define LOTUS_CONV_GENERIC 1      // conv_kernel<128, 64 | 128, fwd | dgrad>
#define LOTUS_CONV_STEM 2         // conv_smallcin_kernel<CIN>
#define LOTUS_CONV_PAIRS 3        // conv_pairs_kernel<NCS, PREC> (+ conv_part_reduce_kernel when nz > 1)
#define LOTUS_CONV_OS 4           // conv_os_kernel<PREC, NS, KCH> (+ conv_part_reduce_kernel when nz > 1)
#define LOTUS_CONV_TAP 5          // gemm_dma_tap_kernel / gemm_kernel over the tap plan + conv_tap_reduce_kernel
#define LOTUS_CONV_WGRAD 6        // conv_wgrad_kernel<64 | 128, 64 | 128>
#define LOTUS_CONV_WGRAD_BF16 7   // conv_wgrad_bf16_kernel<PREC>
#define LOTUS_CONV_WGRAD_STEM 8   // conv_smallcin_wgrad_kernel

extern __attribute__((visibility("hidden"))) __thread int lotus_tls_conv_route[8];
static inline void lotus_note_conv_route(int family, int mode, int rows, int cols, int prec, int nz, int tpz, int aux) {
  int* r = lotus_tls_conv_route;
  r[0] = family; r[1] = mode; r[2] = rows; r[3] = cols; r[4] = prec; r[5] = nz; r[6] = tpz; r[7] = aux;
}
