// Headers that the device kernels and the host-only translation unit (mpfmt_host.cpp, also built by g++ for the sanitizer tests) share
// keep their HIP function qualifiers; where the HIP runtime header has not defined them (a plain C++ compiler, or a host file that
// does not include it) they mean nothing more than `inline`.
#pragma once
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#ifndef __forceinline__
#define __forceinline__ inline __attribute__((always_inline))
#endif
