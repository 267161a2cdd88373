// rt_gemm_skinny_bf16 — C = lo·Wᵀ + (hi·Wᵀ + bias) for M <= 32 rows: the adaLN tables (mmdit.ModulationTable), M = steps·batch.
//
// A weight-streaming job: every W byte is used once, so W goes global -> register -> v_mfma_f32_16x16x32_bf16 with no LDS stage, and
// each W fragment feeds BOTH products (the hi and the lo half of the two-term bf16 split of silu(temb)); the 256x256-tile kernel
// ran the same table as two launches of N/256 workgroups that each walked K serially and streamed W twice.
//
// One wave per 16 output columns, NW waves (16·NW columns) per workgroup, the whole K in one accumulator chain per product. The
// activations are the part that IS reused — every wave needs all of hi and lo (4x the bytes of its own W slice at M = 32) — so a
// workgroup stages them once per 256-element K stage in LDS (double buffered, 2 x 32 KiB) and its waves read their MFMA operands
// from there; W is prefetched two stages ahead in registers and stays in flight across the stage barrier (rt_lds_barrier orders LDS
// traffic only). Without the LDS stage every wave re-read hi/lo through L2 and the kernel ran at the L2 rate (1.5 TB/s of W).
// LDS image of a stage: [hi|lo][row][512 B], 16-byte chunk c of row r at c ^ (r & 15): the 16 rows a lane group reads at one
// logical chunk land on 16 distinct slots of the 256-byte bank row.
//
// Bit-identical to rt_gemm_bf16(hi, bias) followed by rt_gemm_bf16(lo, res = C):
//   * same instruction, same operand roles (W rows = A operand, activation rows = B operand), K ascending in steps of 32, and lane
//     group j = lane >> 4 holds k = 32s + 8j .. +7 of step s — what gemm_tile's chunk swizzle hands the MFMA;
//   * the epilogue repeats epilogue_tile's operations: (acc_hi + bias) · 1.0 (the fp32 value the first launch stores), then
//     (acc_lo + 0) · 1.0 + that.
// Rows >= M of a fragment read row M-1 (as gemm_tile clamps) and are not stored; an MFMA output row depends on its own operand row only.
#include "rt_common.h"

namespace {

constexpr int SK_U = 8;            // k-steps (of 32) per stage: 256 elements = 512 B per activation row
constexpr int SK_MAX_GROUPS = 2;
// waves per workgroup = waves that share one LDS copy of the activations. Measured at 28x9216x3072 (144 workgroups of 4 waves):
// 4 waves 24.9 us, 2 waves (288 workgroups, twice the activation traffic) 27.3 us; at 28x18432x3072 x2: 72 vs 75 us.
constexpr int SK_NW = 4;

struct SkinnyLaunch {
  rt_skinny_group g[SK_MAX_GROUPS];
  int wg_begin[SK_MAX_GROUPS];
  const bf16_t* hi;
  const bf16_t* lo;
  int64_t lda;
  int M, K, ngroups;
};

template <int MF, int NW>   // MF m-fragments of 16 rows: 1 (M <= 16) or 2; NW waves per workgroup
__global__ __launch_bounds__(64 * NW) void gemm_skinny_kernel(const SkinnyLaunch L) {
  constexpr int ROWS = 16 * MF;
  constexpr int HALF = ROWS * 512;                   // bytes of hi (or lo) per stage
  constexpr int BUF = 2 * HALF;
  constexpr int NLD = 2 * ROWS * 32 / (64 * NW);     // 16-byte chunks per thread and stage
  static_assert(NLD * 64 * NW == 2 * ROWS * 32, "the stage is dealt evenly over the workgroup");
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int gi = 0, wg = (int)blockIdx.x;
  if (L.ngroups > 1 && wg >= L.wg_begin[1]) { gi = 1; wg -= L.wg_begin[1]; }
  const rt_skinny_group& g = L.g[gi];
  const int r = lane & 15, kc = (lane >> 4) * 8;
  const int frag = wg * NW + wave;
  const bool active = frag * 16 < g.N;               // the last workgroup of a problem may have idle waves: they stage and meet, only
  const int n0 = active ? frag * 16 : 0;             // (N % 16 == 0, host check)
  const bf16_t* wp = reinterpret_cast<const bf16_t*>(g.W) + (int64_t)(n0 + r) * g.ldw + kc;

  // staging: chunk idx = i*64*NW + tid -> (hi|lo, row, 16-byte chunk c of the stage's 512-byte row)
  const bf16_t* asrc[NLD];
  int adst[NLD];
#pragma unroll
  for (int i = 0; i < NLD; ++i) {
    const int idx = i * 64 * NW + tid;
    const int which = idx / (ROWS * 32), row = (idx >> 5) % ROWS, c = idx & 31;
    asrc[i] = (which ? L.lo : L.hi) + (int64_t)min(row, L.M - 1) * L.lda + c * 8;
    adst[i] = which * HALF + row * 512 + ((c ^ (row & 15)) << 4);
  }
  u32x4 areg[NLD];
  auto load_a = [&](int k) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) areg[i] = *reinterpret_cast<const u32x4*>(asrc[i] + k);
  };
  auto store_a = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) *reinterpret_cast<u32x4*>(smem + buf * BUF + adst[i]) = areg[i];
  };
  struct WStage { bf16x8 w[SK_U]; };
  auto load_w = [&](WStage& s, int k) {
#pragma unroll
    for (int u = 0; u < SK_U; ++u) s.w[u] = *reinterpret_cast<const bf16x8*>(wp + k + 32 * u);
  };

  f32x4 acc_h[MF], acc_l[MF];
#pragma unroll
  for (int f = 0; f < MF; ++f) acc_h[f] = acc_l[f] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int rd = r * 512;                            // + f*8192 + which*HALF + (((4u + j) ^ r) << 4)
  const int j4 = lane >> 4;
  auto mma = [&](const WStage& s, int buf) {
    const char* tb = smem + buf * BUF + rd;
#pragma unroll
    for (int u = 0; u < SK_U; ++u) {
      const int co = ((4 * u + j4) ^ r) << 4;
#pragma unroll
      for (int f = 0; f < MF; ++f) {
        const bf16x8 h = *reinterpret_cast<const bf16x8*>(tb + f * 8192 + co);
        const bf16x8 l = *reinterpret_cast<const bf16x8*>(tb + HALF + f * 8192 + co);
        acc_h[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(s.w[u], h, acc_h[f], 0, 0, 0);
        acc_l[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(s.w[u], l, acc_l[f], 0, 0, 0);
      }
    }
  };

  // K % 256 == 0 (host check). Stage s: activations of s+1 and W of s+2 are requested, then the MFMAs of s, then s+1's activations
  // go to the other LDS buffer (last read in stage s-1, i.e. before the previous barrier) and the workgroup meets.
  constexpr int KS = 32 * SK_U;
  const int K = L.K;
  // W lives in three register stages used in rotation (stage s computes from ring[s % 3] and requests s+2 into ring[(s+2) % 3]); the
  // rotation is spelled out so that no register moves — which would wait for the youngest loads — are needed.
  WStage w0, w1, w2;
  int k = 0, buf = 0;
  // Both requests of a stage are unconditional (the last stages re-request W's final stage instead of branching): the compiler's
  // vmcnt bookkeeping then knows that the W loads are younger than the activation loads and lets them stay in flight while the
  // activations are written to LDS.
  auto stage = [&](const WStage& cur, WStage& far) {         // a stage that has a successor
    load_a(k + KS);
    load_w(far, min(k + 2 * KS, K - KS));
    mma(cur, buf);
    store_a(buf ^ 1);
    rt_lds_barrier();
    k += KS;
    buf ^= 1;
  };
  load_a(0);
  load_w(w0, 0);
  load_w(w1, min(KS, K - KS));
  store_a(0);
  rt_lds_barrier();
  for (;;) {
    if (k + KS >= K) { mma(w0, buf); break; }
    stage(w0, w2);
    if (k + KS >= K) { mma(w1, buf); break; }
    stage(w1, w0);
    if (k + KS >= K) { mma(w2, buf); break; }
    stage(w2, w1);
  }

  // lane owns row m = 16f + r and the 4 consecutive columns n .. n+3
  const int n = n0 + 4 * (lane >> 4);
  f32x4 bias4 = f32x4{0.f, 0.f, 0.f, 0.f};
  if (g.bias) {
    const u32x2 b = *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16_t*>(g.bias) + n);
    bias4 = f32x4{bf16lo(b[0]), bf16hi(b[0]), bf16lo(b[1]), bf16hi(b[1])};
  }
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int f = 0; f < MF; ++f) {
    const int m = 16 * f + r;
    f32x4 first = acc_h[f] + bias4;      // launch 1 of the pair: v = acc + bias; v *= alpha (1.0); stored as fp32
    first *= 1.0f;
    f32x4 v = acc_l[f] + zero4;          // launch 2: v = acc + (no bias = 0); v *= 1.0; v += res
    v *= 1.0f;
    v += first;
    if (active && m < L.M) *reinterpret_cast<f32x4*>(g.C + (int64_t)m * g.ldc + n) = v;
  }
}

}  // namespace

extern "C" int rt_gemm_skinny_bf16(const void* hi, const void* lo, int64_t lda, int32_t M, int32_t K, const rt_skinny_group* groups,
                                   int32_t ngroups, void* stream) {
  if (!hi || !lo || !groups || ngroups < 1 || ngroups > SK_MAX_GROUPS || M < 1 || K < 1) return RT_E_BADARG;
  if (M > 32 || K % (32 * SK_U) != 0) return RT_E_SHAPE;
  if (!RT_ALIGNED(hi, 16) || !RT_ALIGNED(lo, 16) || lda % 8) return RT_E_ALIGN;
  if (lda < K) return RT_E_SHAPE;
  SkinnyLaunch L{};
  L.hi = (const bf16_t*)hi;
  L.lo = (const bf16_t*)lo;
  L.lda = lda;
  L.M = M;
  L.K = K;
  L.ngroups = ngroups;
  for (int i = 0; i < ngroups; ++i) {
    const rt_skinny_group& g = groups[i];
    if (!g.W || !g.C || g.N < 1) return RT_E_BADARG;
    if (g.N % 16 != 0 || g.ldw < K || g.ldc < g.N) return RT_E_SHAPE;
    if (!RT_ALIGNED(g.W, 16) || g.ldw % 8 || !RT_ALIGNED(g.C, 16) || g.ldc % 4) return RT_E_ALIGN;
    if (g.bias && !RT_ALIGNED(g.bias, 8)) return RT_E_ALIGN;
    L.g[i] = g;
  }
  int total = 0;
  for (int i = 0; i < ngroups; ++i) {
    L.wg_begin[i] = total;
    total += (groups[i].N / 16 + SK_NW - 1) / SK_NW;
  }
  hipStream_t st = (hipStream_t)stream;
  if (M <= 16) hipLaunchKernelGGL((gemm_skinny_kernel<1, SK_NW>), dim3(total), dim3(64 * SK_NW), 0, st, L);
  else hipLaunchKernelGGL((gemm_skinny_kernel<2, SK_NW>), dim3(total), dim3(64 * SK_NW), 0, st, L);
  return rt_hip_status();
}
