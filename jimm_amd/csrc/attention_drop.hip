// The attention-dropout instantiations (template flag DROP) of the forward and
// backward flash kernels, as one translation unit of their own: it includes
// attention.hip and attention_bwd_fused.hip, whose host sections then define
// only the DROP launchers attn_fwd_drop and attn_bwd_drop.
//
// fp32 arithmetic is not to be packed in pairs (v_pk_*_f32) in the new
// instantiations, while the DROP-off kernels keep the code they have always
// compiled to; so the setting covers this unit's device pass, helpers of
// common.h and mfma.h included (one setting for all of them, or they would
// not be inlined), and nothing of the two original units.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#define JIMM_ATTN_DROP_TU 1

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "attention.hip"
#include "attention_bwd_fused.hip"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
