// pa_hd.h -- PA_HD: how a function is declared that is stated once for the kernels and for their host twins.
#pragma once

#if defined(__HIPCC__)
#define PA_HD __host__ __device__ __forceinline__
#else
#define PA_HD inline
#endif
