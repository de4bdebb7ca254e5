// bf16 twin of attn_grad.hip (see bf16_names.h)
#include "bf16_names.h"
#include "attn_grad.hip"
