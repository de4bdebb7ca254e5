// bf16 twin of relayout.hip: the same kernel with bf16 storage (dadd_common.h), named *_bf16 (bf16_names.h).  The host-only
// planning functions exist once, in the fp16 build.
#include "bf16_names.h"
#include "relayout.hip"
