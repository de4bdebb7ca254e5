// bf16 twin of plan_refresh.hip: the same kernel with bf16 destinations (dadd_common.h), named *_bf16 (bf16_names.h).  The
// host-only planning functions exist once, in the fp16 build.
#include "bf16_names.h"
#include "plan_refresh.hip"
