// Diagnostic copy of the library's GEMM (csrc/gemm_bf16.hip, included below with its two hooks defined): every wave takes s_memtime
// at the end of the K loop (t0), behind the last store of its epilogue (t1) and, after s_waitcnt vmcnt(0), at its end (t2), and lane 0
// writes them to a buffer of their own — 8 x 8 bytes per wave at ((block * 8 + wave) * 8): t0, t1, t2, epilogue kind, and
// s_memrealtime (100 MHz) at t0 and t2 to convert s_memtime ticks into time. t1 - t0 is what the epilogue takes to ISSUE, t2 - t1 what
// is left of the memory system DRAINING once nothing more is issued. The stamps cost a few scalar instructions and one 64-byte store
// per wave; the K loop is the library's. Not part of librt_reptext_hip.so: built by the Makefile beside this file and driven by
// report.py. Timings of this build are for the split only, never for a comparison of kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ uint64_t* rt_stamp_buf;

__device__ __forceinline__ void rt_stamp_write(uint64_t t0, uint64_t r0, int kind) {
  __builtin_amdgcn_sched_barrier(0);
  const uint64_t t1 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const uint64_t t2 = __builtin_amdgcn_s_memtime();
  const uint64_t r2 = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_sched_barrier(0);
  uint64_t* b = rt_stamp_buf;
  if (b && (threadIdx.x & 63) == 0) {
    uint64_t* p = b + ((size_t)blockIdx.x * 8 + (threadIdx.x >> 6)) * 8;
    p[0] = t0; p[1] = t1; p[2] = t2; p[3] = (uint64_t)kind; p[4] = r0; p[5] = r2;
  }
}

#define RT_GEMM_STAMP_KLOOP_END()                                  \
  __builtin_amdgcn_sched_barrier(0);                               \
  const uint64_t rt_stamp_t0 = __builtin_amdgcn_s_memtime();       \
  const uint64_t rt_stamp_r0 = __builtin_amdgcn_s_memrealtime();   \
  __builtin_amdgcn_sched_barrier(0)
#define RT_GEMM_STAMP_STORES_ISSUED(kind) rt_stamp_write(rt_stamp_t0, rt_stamp_r0, (kind))

#include "gemm_bf16.hip"

// Stamps of the launches that follow go to `dev` (device memory, 64 bytes per wave = 512 per workgroup of the largest launch); NULL: none.
extern "C" int rt_gemm_stamps_buffer(uint64_t* dev) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(rt_stamp_buf), &dev, sizeof(dev));
}
