// Shared between the fp32 weight-gradient kernels (conv_wgrad.hip, conv_wgrad_wino.hip).  gfx950 only.
#pragma once
#include "shg_device.h"

// conv_wgrad.hip: dw[e] = sum over the nslice partial tensors part[slice][e], e < n, in slice order (deterministic, no atomics)
void shg_launch_wgrad_reduce(const float* part, float* dw, long n, int nslice, hipStream_t s);
