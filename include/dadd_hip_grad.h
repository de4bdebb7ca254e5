/*
 * dadd_hip_grad.h - the part of libdadd_hip.so's C ABI that only a training backward needs and that has no place in the
 * sampler's header: the bf16 sibling of the weight-gradient entry point.  Conventions, status codes and the descriptor
 * are those of dadd_hip.h (dadd_wgrad_desc, next to the fp16 form of the same call).
 */
#ifndef DADD_HIP_GRAD_H
#define DADD_HIP_GRAD_H

#include "dadd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The contract of the fp16 weight-gradient entry point of dadd_hip.h with dy and x in bf16 (round to nearest even on the
 * way in is the caller's; fp32 accumulation, fp32 dw / dbias): the weight-gradient kernel compiled for bf16 storage
 * (csrc/wgrad_bf16.hip), for the UNet's bf16 operand mode. */
int dadd_conv_wgrad_bf16(const dadd_wgrad_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DADD_HIP_GRAD_H */
