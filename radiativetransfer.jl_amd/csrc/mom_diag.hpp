// mom_diag.hpp -- diagnostic builds only (make EXTRA=-DMOM_DIAG_STAMPS): s_memtime deltas of the middle
// workgroup, lane 0 of wave 0 (MOM_STAMP) and of wave 4 (MOM_STAMP4), accumulated per code section; each
// translation unit has its own accumulators and reader.  Never part of the shipped library.
#pragma once
#ifdef MOM_DIAG_STAMPS
#include <hip/hip_runtime.h>
static __device__ unsigned long long mom_diag_acc[128];
static __device__ unsigned long long mom_diag_last, mom_diag_last4;
__device__ __forceinline__ unsigned long long mom_diag_now() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#define MOM_STAMP_(id, tid, last)                                        \
  do {                                                                   \
    __builtin_amdgcn_sched_barrier(0);                                   \
    if (threadIdx.x == (tid) && blockIdx.x == (gridDim.x >> 1)) {        \
      unsigned long long n__ = mom_diag_now();                           \
      mom_diag_acc[id] += n__ - last;                                    \
      last = n__;                                                        \
    }                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                   \
  } while (0)
#define MOM_STAMP(id) MOM_STAMP_(id, 0, mom_diag_last)
#define MOM_STAMP4(id) MOM_STAMP_(id, 256, mom_diag_last4)
#endif
// -DMOM_DIAG_TIMELINE (the two-buffer strip image, tools/phase_stamps_s2.py): instead of sums per section, a TIMELINE per
// workgroup on the constant 100 MHz clock (s_memrealtime: one clock for all CUs), so that the sections of the two workgroups that
// share a CU can be laid over each other.  Lane 0 of wave 0 of every workgroup appends (clock << 4 | id of the section that has
// just ended) from the workgroup's SECOND unit on (steady state), up to kTlCap events; the count lives in the LDS int c.ipiv[2],
// which the two-buffer image does not use otherwise.  mom_tl_hdr[4 b ..]: CU key, arrival ticket on the CU, favoured, events.
#ifdef MOM_DIAG_TIMELINE
#include <hip/hip_runtime.h>
constexpr int kTlWgs = 512, kTlCap = 2048;
static __device__ unsigned long long mom_tl_ev[(size_t)kTlWgs * kTlCap];
static __device__ unsigned mom_tl_hdr[kTlWgs * 4];
#define MOM_TL(c, id)                                                                        \
  do {                                                                                       \
    if (threadIdx.x == 0 && blockIdx.x < kTlWgs) {                                           \
      const int n__ = (c).ipiv[2];                                                           \
      if (n__ >= 0 && n__ < kTlCap) {                                                        \
        mom_tl_ev[(size_t)blockIdx.x * kTlCap + n__] = (wall_clock64() << 4) | (unsigned)(id); \
        (c).ipiv[2] = n__ + 1;                                                               \
      }                                                                                      \
    }                                                                                        \
  } while (0)
#else
#define MOM_TL(c, id)
#endif
