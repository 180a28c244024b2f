// rtx_limits.h — the plain constants the kernels and the host's launch plan (rtx_plan.h) both need: no types, nothing of HIP.
#pragma once

#define RTX_MAX_LEVELS   12          // NUMBER_OF_BOUNCES + 1 wavefront levels supported
#define RTX_WAVE         64
#ifndef RTX_PK_BLOCK
#define RTX_PK_BLOCK    64           // the waves of a packet launch are independent: one wave per workgroup finds room beside other frames' kernels
                                     // soonest (with k_items at 64 too: 1.318 -> 1.275 ms per frame; either one alone: no change)
#endif
#define RTX_PK_STACK    64           // packet stack entries per wave = lanes of the stack VGPRs
