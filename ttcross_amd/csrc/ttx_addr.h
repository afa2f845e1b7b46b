// ttx_addr.h -- where the per-group, per-bond arrays of DevProb (ttx_dev.h) keep core p and bond s of group g.
#pragma once
#include <hip/hip_runtime.h>
#include "ttx_dev.h"

__device__ __forceinline__ double *core_ptr(const DevProb &P, double *base, int g, int p, int first)
{ return base + ((size_t)g * P.NC + (p - first)) * P.CS; }
__device__ __forceinline__ double *inv_ptr(const DevProb &P, int g, int s, int first)   // bond s in first-1..last
{ return P.inv + ((size_t)g * P.NC + (s - first + 1)) * (size_t)P.RM * P.RM; }
__device__ __forceinline__ int *vip_ptr(const DevProb &P, int g, int s, int first)
{ return P.vip + ((size_t)g * P.NC + (s - first + 1)) * (size_t)4 * P.RM; }
__device__ __forceinline__ short *L_ptr(const DevProb &P, int g, int s, int first)      // bond s in first-1..last
{ return P.L + ((size_t)g * P.NC + (s - first + 1)) * (size_t)P.d * P.RM; }
__device__ __forceinline__ short *R_ptr(const DevProb &P, int g, int s, int first)      // bond s in first..last+1
{ return P.R + ((size_t)g * P.NC + (s - first)) * (size_t)P.d * P.RM; }
