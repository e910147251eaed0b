// lotus-hip: the launch of the LDS-DMA dense kernels (gemm_dma.h).  Which products they take, and on which tile, is decided by
// gemm_route (gemm.hip); this is its own translation unit because it is compiled with -mllvm -amdgpu-mfma-vgpr-form
// (accumulators in VGPRs: the epilogue stores straight from them); gemm.hip keeps the default register form for the kernels
// that were tuned with it.
#include "gemm_dma.h"

namespace LOTUS_NS {

// Every gemm_dma_kernel instantiation of the library is named in dma_go, every gemm_dma_tap_kernel in dma_tap_go.  The epilogues:
// the LayerNorm backward (2) exists for the input gradient, the full epilogue (1) not for weight gradients (they have none).
template <int BM, int BN, int BK, int NST, bool XKC, bool WKC, bool SUM_A>
static void dma_go(const GemmRoute& r, const GemmP& p, hipStream_t st) {
  const dim3 block(256);
  if constexpr (XKC && !WKC) {
    if (r.epi == 2) { LOTUS_LAUNCH((gemm_dma_kernel<BM, BN, BK, NST, XKC, WKC, SUM_A, 2>), r.grid, block, 0, st, p); return; }
  }
  if constexpr (!SUM_A) {
    if (r.epi == 1) { LOTUS_LAUNCH((gemm_dma_kernel<BM, BN, BK, NST, XKC, WKC, SUM_A, 1>), r.grid, block, 0, st, p); return; }
  }
  LOTUS_LAUNCH((gemm_dma_kernel<BM, BN, BK, NST, XKC, WKC, SUM_A, 0>), r.grid, block, 0, st, p);
}
template <bool XKC, bool WKC, bool SUM_A>
static void dma_go_tile(const GemmRoute& r, const GemmP& p, hipStream_t st) {
  if (r.bm == 128 && r.bn == 128) dma_go<128, 128, 16, 3, XKC, WKC, SUM_A>(r, p, st);
  else if (r.bm == 128) dma_go<128, 64, 32, 2, XKC, WKC, SUM_A>(r, p, st);
  else if constexpr (SUM_A) {  // 64-row tiles: weight gradients dW of <= 64 rows
    if (r.bn == 128) dma_go<64, 128, 32, 2, XKC, WKC, SUM_A>(r, p, st);
    else dma_go<64, 64, 32, 3, XKC, WKC, SUM_A>(r, p, st);
  }
}
template <bool WKC>
static void dma_tap_go(const GemmRoute& r, const GemmP& p, hipStream_t st) {
  if (r.bn == 128) LOTUS_LAUNCH((gemm_dma_tap_kernel<128, 128, 16, 3, WKC>), r.grid, dim3(256), 0, st, p);
  else LOTUS_LAUNCH((gemm_dma_tap_kernel<128, 64, 32, 2, WKC>), r.grid, dim3(256), 0, st, p);
}

// the launch of a family-2 / family-3 route (fp32 storage only: gemm_route gives the bf16-storage build neither)
int gemm_dma_launch(const GemmRoute& r, const GemmP& p, hipStream_t st) {
  if constexpr (LOTUS_ACT_IS_BF16) {
    lotus_set_error("lotus_gemm(dma): not built for bf16 activation storage");
    return LOTUS_E_UNSUPPORTED;
  } else {
    gemm_note(r);
    if (r.family == 3) {
      if (r.layout == GEMM_FWD) dma_tap_go<true>(r, p, st);
      else dma_tap_go<false>(r, p, st);
    } else if (r.layout == GEMM_FWD) dma_go_tile<true, true, false>(r, p, st);
    else if (r.layout == GEMM_DGRAD) dma_go_tile<true, false, false>(r, p, st);
    else dma_go_tile<false, false, true>(r, p, st);
    LOTUS_LAUNCH_CHECK(r.name);
    return LOTUS_OK;
  }
}

}  // namespace LOTUS_NS
