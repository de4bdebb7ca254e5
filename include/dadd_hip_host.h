/*
 * dadd_hip_host.h - host-only entry points of libdadd_hip.so beside include/dadd_hip.h (bound through
 * lib.HOST_PROTOTYPES): no launch, no HIP call, usable without a GPU.
 */
#ifndef DADD_HIP_HOST_H
#define DADD_HIP_HOST_H

#include "dadd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dadd_conv_igemm_resolve_f16 for the bf16 build: what dadd_conv_igemm_bf16 would launch (the *_bf16 kernel names). */
int dadd_conv_igemm_resolve_bf16(const dadd_igemm_desc* d, int num_cu, dadd_igemm_choice* out);

#ifdef __cplusplus
}
#endif

#endif
