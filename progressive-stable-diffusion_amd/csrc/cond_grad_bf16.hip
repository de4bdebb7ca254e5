// bf16 twin of cond_grad.hip: the same kernels with bf16 storage (dadd_common.h), named *_bf16 (bf16_names.h).
#include "bf16_names.h"
#include "cond_grad.hip"
