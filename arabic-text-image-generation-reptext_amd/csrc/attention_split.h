// Key-split tail of the two bf16 attention kernels (attention.hip: 128-row items, two workgroups per CU; attention_v3.hip:
// 256-row items, one per CU), defined ONCE: the cut, the runs, the parts of a split item, the record index, the ticket.
// Each kernel file keeps its item height, workgroups per CU, record payload and combine arithmetic.
//
// With NI items per XCD group on `spx` workgroups, the last NI mod spx items would occupy a partial round of full-length
// workgroups (864 items on 512 slots: 1.69 rounds run as 2). Instead those `rem` items × ntiles key tiles are dealt to the
// `spx` workgroups in equal contiguous runs of tiles; a run covers the tail of one item and/or the head of the next (never
// more: a run is shorter than an item because rem < spx). A workgroup that covers only part of an item writes its
// unnormalised partial to a workspace record (write-through stores, layout owned by the kernel) and takes a ticket on the
// item's counter; the workgroup that draws the last ticket combines the item's records IN RUN ORDER (not arrival order:
// bitwise reproducible) and stores the output. The decomposition depends on (S, H, CU count) only — every batch entry is
// cut identically, so results do not depend on the batch size.
#pragma once
#include "rt_common.h"

constexpr int CNT_ALIGN = 256;       // the records start at this alignment behind the counters
constexpr int SPLIT_MIN_TILES = 8;   // do not split runs shorter than this many key tiles

struct SplitGeom {               // kernel argument of both kernels: keep the field order
  int S, H, nqb, ntiles, NI;     // NI = H * nqb work items per batch entry
  int spx;                       // workgroups per XCD group that take items side by side
  int split;                     // key-split tail enabled (workspace present)
};

// How the items of one XCD group are cut (identical on host and device; scalar arithmetic only).
struct GroupCut {
  int start, cnt;   // first item and number of items of this group
  int nfull;        // items run whole by one workgroup each
  int rem;          // items whose key tiles are dealt to the `spx` workgroups (0: no split)
};
__host__ __device__ inline GroupCut group_cut(const SplitGeom& G, int xcd) {
  GroupCut c;
  const int base = G.NI >> 3, extra = G.NI & 7;
  c.cnt = base + (xcd < extra ? 1 : 0);
  c.start = xcd * base + (xcd < extra ? xcd : extra);
  c.nfull = c.cnt;
  c.rem = 0;
  if (G.split) {
    const int nf = (c.cnt / G.spx) * G.spx, rem = c.cnt - nf;
    // split when the partial round is less than 15/16 full and every run keeps >= SPLIT_MIN_TILES tiles
    if (rem > 0 && rem * 16 < G.spx * 15 && (int64_t)rem * G.ntiles >= (int64_t)G.spx * SPLIT_MIN_TILES) {
      c.nfull = nf;
      c.rem = rem;
    }
  }
  return c;
}

// Run of splitting workgroup j (0 <= j < spx) of a group with cut.rem > 0: key tiles [lo, hi) counted through the group's
// split items laid end to end; i0 = the first of those items it touches (the run may continue into item i0 + 1).
// 32-bit arithmetic: the host checks split_fits_32bit.
struct SplitRun { int lo, hi, i0; };
__device__ __forceinline__ SplitRun split_run(const SplitGeom& G, const GroupCut& cut, int j) {
  const unsigned U = (unsigned)cut.rem * (unsigned)G.ntiles;
  SplitRun r;
  r.lo = (int)((unsigned)j * U / (unsigned)G.spx);
  r.hi = (int)((unsigned)(j + 1) * U / (unsigned)G.spx);
  r.i0 = r.lo / G.ntiles;
  return r;
}

// The splitting workgroups j_first..j_last that cover split item `ritem` (index among the group's split items): the same
// closed forms on every workgroup.
struct SplitParts {
  unsigned U, a;   // tiles of all split items of the group; first tile of this item
  int j_first, j_last, nparts;
};
__device__ __forceinline__ SplitParts split_parts(const SplitGeom& G, const GroupCut& cut, int ritem) {
  const unsigned U = (unsigned)cut.rem * (unsigned)G.ntiles, spx = (unsigned)G.spx;
  const unsigned a = (unsigned)ritem * (unsigned)G.ntiles, bnd = a + (unsigned)G.ntiles;
  SplitParts p;
  p.U = U;
  p.a = a;
  p.j_first = (int)(((a + 1) * spx + U - 1) / U) - 1;
  p.j_last = min(G.spx - 1, (int)((bnd * spx + U - 1) / U) - 1);
  p.nparts = p.j_last - p.j_first + 1;
  return p;
}
// Which of workgroup j's two segments holds the item: the second when the item starts after the run does.
__device__ __forceinline__ int split_seg_of(const SplitGeom& G, const SplitParts& p, int j) {
  const unsigned lo_j = (unsigned)j * p.U / (unsigned)G.spx;
  return (p.a > lo_j) ? 1 : 0;
}
// Index of the record of (batch entry, XCD group, splitting workgroup, segment); times the kernel's record size = byte offset.
__device__ __forceinline__ int64_t split_rec_index(const SplitGeom& G, int b, int xcd, int j, int seg) {
  return (((int64_t)b * 8 + xcd) * G.spx + j) * 2 + seg;
}

// Ticket on a split item's counter, taken by a workgroup that has just issued the write-through stores of its record.
// Returns (wave-uniform) whether this workgroup drew the last of the item's `nparts` tickets and so combines the records.
// `flag` is an LDS word nobody else uses until the next barrier after the return.
//   1. every wave drains its stores (vmcnt(0)) and the workgroup meets: the whole record has left for memory;
//   2. thread 0 adds 1 to the counter (relaxed, agent scope — the stores before it were write-through and drained, so no
//      release is needed to make them visible at the agent's coherence point);
//   3. the holder of the last ticket resets the counter to 0 — the workspace is zero at rest, ready for the next launch,
//      and no other workgroup touches this counter any more — then drops this CU's stale lines (acquire fence) and waits
//      for the invalidate before anybody reads a record;
//   4. the verdict goes through LDS and a barrier to the other waves.
// Nobody waits on anybody: a workgroup that is not last leaves, so no assumption on dispatch order or co-residency exists.
__device__ __forceinline__ bool split_ticket(int* cnt, int nparts, volatile int* flag, int tid) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const int old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = (old == nparts - 1) ? 1 : 0;
    if (last) {
      __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *flag = last;
  }
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(*flag) != 0;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// CUs of the current device; 256 (MI355X) when there is none to ask.
inline int split_cu_count() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
  }
  return cus;
}
// Geometry for items of `bq` query rows and key tiles of `bkv` keys on `spx` workgroups per XCD group.
inline SplitGeom split_geom(int S, int H, int bq, int bkv, int spx, bool split) {
  const int nqb = (S + bq - 1) / bq;
  return SplitGeom{S, H, nqb, (S + bkv - 1) / bkv, H * nqb, spx > 0 ? spx : 1, split ? 1 : 0};
}
// The run arithmetic above stays below 2^31
inline bool split_fits_32bit(const SplitGeom& G) { return (int64_t)G.NI * (G.ntiles + 1) * G.spx < ((int64_t)1 << 31); }
inline bool split_any(const SplitGeom& G) {   // does any XCD group split?
  bool any = false;
  for (int x = 0; x < 8; ++x) any = any || group_cut(G, x).rem > 0;
  return any;
}
// The counter region is laid out for 128-row items (attention.hip's; attention_v3.hip has half as many), one int each, so one
// workspace serves either kernel: both keep their counters inside it (zero at rest) and their records behind it.
inline int64_t split_cnt_bytes(int B, int S, int H) {
  return (((int64_t)B * H * ((S + 127) / 128) * 4 + CNT_ALIGN - 1) / CNT_ALIGN) * CNT_ALIGN;
}
// Workspace of a kernel with records of `rec_bytes` per (workgroup, segment): counters, then two records per splitting
// workgroup. 0 when no XCD group of this geometry splits.
inline int64_t split_ws_bytes(int B, const SplitGeom& G, int64_t rec_bytes) {
  if (!split_any(G)) return 0;
  return split_cnt_bytes(B, G.S, G.H) + (int64_t)B * 8 * G.spx * 2 * rec_bytes;
}

// ---- attention_v3.hip, as seen by the front end rt_attention_fwd (attention.hip) -------------------------------------------------
// Workspace attention_v3 wants for (B, S, H); 0 when nothing would be split or the shape is not its.
int64_t rt_attention_v3_ws_bytes(int32_t B, int32_t S, int32_t H);
// Offers the launch to attention_v3. *taken = 1: the shape is attention_v3's and the return value (RT_OK, RT_E_* or a hipError_t)
// is the launch's status; *taken = 0 (with RT_OK): left to attention.hip.
int rt_attention_v3_try(const void* q, const void* k, const void* v, void* o, int64_t ld, int64_t stride_b, int64_t ldo, int64_t stride_ob,
                        int32_t B, int32_t S, int32_t H, float scale, int32_t row_lo, int32_t row_hi, void* ws, int64_t ws_bytes, void* stream,
                        int* taken);   // [row_lo, row_hi): only the items that hold a query row of this range are computed
int rt_attention_v3_mode(int mode);
