// bf16 twin of wgrad.hip: the same kernels with bf16 storage (dadd_common.h), named *_bf16 (bf16_names.h).
#include "bf16_names.h"
#include "wgrad.hip"
