// bf16 twin of rows_grad.hip: its 16-bit kernels (rowvec_grad) with bf16 storage (dadd_common.h), named *_bf16
// (bf16_names.h).  The fp32 kernels of the row path exist once, in the fp16 build.
#include "bf16_names.h"
#include "rows_grad.hip"
