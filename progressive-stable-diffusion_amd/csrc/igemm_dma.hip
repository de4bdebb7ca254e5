// Implicit-GEMM convolution / linear with LDS-DMA staging: the kernels of igemm_dma_kernel.h's ring for plain convs and
// linears (UPS false) and the nearest-2x upsample as a 9-tap gather (UPS true), their table and its lookup.
#include "igemm_dma_kernel.h"

namespace {

// kernel table (igemm_args.h): BM, BN, UPS, PERS, LNK.  Plain linears / convs and (no upsample) their LayerNorm-folded
// twins; LNK 2 exists on the 128-row tiles only.
#define DMA_ROW(BM, BN, UPS, PERS, LNK)                                                                                \
  {DADD_KNAME("igemm_dma_kernel") "<" #BM ", " #BN ", " #UPS ", " #PERS ", " #LNK ">", igemm_dma_kernel<BM, BN, UPS, PERS, LNK>, \
   512, smem_bytes(BM, BN), {BM, BN, UPS, PERS, LNK}}
#define DMA_ROWS2(BM, BN, PERS) DMA_ROW(BM, BN, false, PERS, 0), DMA_ROW(BM, BN, false, PERS, 1)
#define DMA_ROWS3(BM, BN, PERS) DMA_ROWS2(BM, BN, PERS), DMA_ROW(BM, BN, false, PERS, 2)
const IgemmKernel DMA_KERNELS[] = {
    DMA_ROWS3(128, 128, true),  DMA_ROWS3(128, 160, true),
    DMA_ROWS3(128, 128, false), DMA_ROWS3(128, 160, false),
    DMA_ROW(128, 128, true, false, 0), DMA_ROW(128, 160, true, false, 0),
    DMA_ROWS2(64, 64, false), DMA_ROWS2(64, 128, false), DMA_ROWS2(64, 160, false),
};
#undef DMA_ROWS3
#undef DMA_ROWS2
#undef DMA_ROW

}  // namespace

int dadd_init_igemm_dma() { return dadd_set_max_lds(DMA_KERNELS); }

const IgemmKernel* dadd_igemm_dma_row(int tile_m, int tile_n, bool ups, bool persistent, int lnk) {
  return dadd_find_row(DMA_KERNELS, tile_m, tile_n, ups, persistent, lnk);
}
