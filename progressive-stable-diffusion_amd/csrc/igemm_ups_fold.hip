// The nearest-2x upsample -> 3x3 conv as four 2x2 phase convs on pre-summed weights (dadd_hip.h DADD_TUNE_UPS_FOLD): the
// UPS = 2 mode of the LDS-DMA ring (igemm_dma_kernel.h), K = 4 Cin instead of the gather's 9 Cin.  Non-persistent 128-row
// tiles, as for the gather.
#define DADD_IGEMM_UPS_FOLD      // igemm_dma_kernel.h then defines igemm_ups_fold_kernel<BM, BN>
#include "igemm_dma_kernel.h"

namespace {

// kernel table (igemm_args.h): BM, BN
#define FOLD_ROW(BM, BN) \
  {DADD_KNAME("igemm_ups_fold_kernel") "<" #BM ", " #BN ">", igemm_ups_fold_kernel<BM, BN>, 512, smem_bytes(BM, BN), {BM, BN}}
const IgemmKernel FOLD_KERNELS[] = {FOLD_ROW(128, 128), FOLD_ROW(128, 160)};
#undef FOLD_ROW

}  // namespace

int dadd_init_igemm_ups_fold() { return dadd_set_max_lds(FOLD_KERNELS); }

const IgemmKernel* dadd_igemm_ups_fold_row(int tile_m, int tile_n) { return dadd_find_row(FOLD_KERNELS, tile_m, tile_n); }
