// mhx_hd.h -- the one spelling of "host+device inline function" (MHX_HD) shared by the headers whose logic both the
// kernels and the CPU emulators under tests/emul/ run, and the host stand-in for HIP's uint4.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MHX_HD __host__ __device__ __forceinline__
#else
#define MHX_HD inline
struct uint4 { uint32_t x, y, z, w; };
#endif
