// bf16 twin of igemm_ups_fold.hip: the same kernels with bf16 storage (dadd_common.h), named *_bf16 (bf16_names.h).
#include "bf16_names.h"
#include "igemm_ups_fold.hip"
