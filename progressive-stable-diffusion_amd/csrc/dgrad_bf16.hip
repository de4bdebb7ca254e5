// bf16 twin of dgrad.hip: the same kernel with bf16 storage (dadd_common.h), named *_bf16 (bf16_names.h).
#include "bf16_names.h"
#include "dgrad.hip"
