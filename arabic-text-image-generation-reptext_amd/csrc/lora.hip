// rt_lora_merge_bf16 — W = bf16(W0 + Σ_t scale_t · B_t · A_t): LoRA adapters merged into a bf16 Linear weight on the device.
//
// One workgroup (4 waves) owns a 128 (rows n) x 64 (columns k) tile of W; a wave owns 32 rows x 64 columns. The low-rank product
// runs on v_mfma_f32_16x16x32_bf16 with At (lora_A transposed, [K][r_pad]) as the MFMA A operand and B ([N][r_pad]) as the MFMA B
// operand: both are r-contiguous, so every operand fragment is one 16-byte load straight from global memory (the factors are a few
// MB at most and stay in L2; the W0 read and W write are the HBM traffic). Each term accumulates into its own fp32 tile and is
// added to the running total with one fma by its scale, so W0 + Σ is rounded to bf16 once. The total goes through LDS (fp32,
// row-major per wave) so that W0 is read and W written as 16 bytes per lane along rows. W0 is loaded before the MFMA loop.
#include "rt_common.h"

namespace {

constexpr int kTileN = 128, kTileK = 64, kWaveN = 32, kLdsLd = kTileK + 4;   // +4 floats: the four row groups of a 16-lane write

struct LoraArgs {
  const bf16_t* B[RT_LORA_MAX_TERMS];
  const bf16_t* At[RT_LORA_MAX_TERMS];
  int64_t ldb[RT_LORA_MAX_TERMS], lda[RT_LORA_MAX_TERMS];
  int32_t nj[RT_LORA_MAX_TERMS];   // r_pad / 32
  float scale[RT_LORA_MAX_TERMS];
  const bf16_t* W0;
  bf16_t* W;
  int64_t ld0, ldw;
  int32_t N, K, nterms;
};

__device__ __forceinline__ bf16x8 load8(const bf16_t* p, bool ok) {
  return ok ? *reinterpret_cast<const bf16x8*>(p) : bf16x8{};
}

__global__ __launch_bounds__(256) void lora_merge_kernel(const LoraArgs a) {
  __shared__ float lds[4][kWaveN][kLdsLd];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k0 = blockIdx.x * kTileK;
  const int n0 = blockIdx.y * kTileN + wave * kWaveN;
  // row-contiguous view of the wave's 32 x 64 tile: 8 lanes x 16 bytes per row, 8 rows per pass, 4 passes
  const int rr = lane >> 3, cc = (lane & 7) * 8;
  const bool col_ok = k0 + cc < a.K;      // K % 8 == 0: a 16-byte chunk is wholly inside or wholly outside
  u32x4 w0v[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int n = n0 + p * 8 + rr;
    w0v[p] = (n < a.N && col_ok) ? *reinterpret_cast<const u32x4*>(a.W0 + (int64_t)n * a.ld0 + k0 + cc) : u32x4{};
  }

  f32x4 tot[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) tot[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int l15 = lane & 15, jl = 8 * (lane >> 4);
  bool k_ok[4], n_ok[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) k_ok[i] = k0 + i * 16 + l15 < a.K;
#pragma unroll
  for (int j = 0; j < 2; ++j) n_ok[j] = n0 + j * 16 + l15 < a.N;

  for (int t = 0; t < a.nterms; ++t) {
    const bf16_t* At = a.At[t] + (int64_t)(k0 + l15) * a.lda[t] + jl;
    const bf16_t* Bp = a.B[t] + (int64_t)(n0 + l15) * a.ldb[t] + jl;
    const int64_t da = 16 * a.lda[t], db = 16 * a.ldb[t];
    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int js = 0; js < a.nj[t]; ++js) {
      bf16x8 af[4], bf[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = load8(At + i * da + js * 32, k_ok[i]);
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = load8(Bp + j * db + js * 32, n_ok[j]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    const float s = a.scale[t];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) tot[i][j][e] = __builtin_fmaf(s, acc[i][j][e], tot[i][j][e]);
  }

  // acc[i][j] element e of lane l = delta[n = 16j + (l & 15)][k = 16i + 4(l >> 4) + e]: four consecutive columns of one row
  float (*wl)[kLdsLd] = lds[wave];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) *reinterpret_cast<f32x4*>(&wl[16 * j + l15][16 * i + 4 * (lane >> 4)]) = tot[i][j];
  __syncthreads();

#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int r = p * 8 + rr, n = n0 + r;
    if (n >= a.N || !col_ok) continue;
    u32x4 o = w0v[p];
    if (a.nterms > 0) {       // nterms == 0 stores W0's bits unchanged
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(&wl[r][cc]);
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(&wl[r][cc + 4]);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        o[q] = pack_bf16x2(bf16lo(w0v[p][q]) + x0[2 * q], bf16hi(w0v[p][q]) + x0[2 * q + 1]);
        o[q + 2] = pack_bf16x2(bf16lo(w0v[p][q + 2]) + x1[2 * q], bf16hi(w0v[p][q + 2]) + x1[2 * q + 1]);
      }
    }
    *reinterpret_cast<u32x4*>(a.W + (int64_t)n * a.ldw + k0 + cc) = o;
  }
}

}  // namespace

extern "C" int rt_lora_merge_bf16(const rt_lora_term* terms, int32_t nterms, const void* W0, int64_t ld0, void* W, int64_t ldw,
                                  int32_t N, int32_t K, void* stream) {
  if (!W0 || !W || N < 1 || K < 1 || nterms < 0 || (nterms > 0 && !terms)) return RT_E_BADARG;
  if (nterms > RT_LORA_MAX_TERMS || K % 8) return RT_E_SHAPE;
  if (ld0 < K || ldw < K) return RT_E_BADARG;
  if (!RT_ALIGNED(W0, 16) || !RT_ALIGNED(W, 16) || ld0 % 8 || ldw % 8) return RT_E_ALIGN;
  LoraArgs a = {};
  for (int t = 0; t < nterms; ++t) {
    const rt_lora_term& x = terms[t];
    if (!x.B || !x.At) return RT_E_BADARG;
    if (x.r_pad < 32 || x.r_pad % 32) return RT_E_SHAPE;
    if (x.ldb < x.r_pad || x.lda < x.r_pad) return RT_E_BADARG;
    if (!RT_ALIGNED(x.B, 16) || !RT_ALIGNED(x.At, 16) || x.ldb % 8 || x.lda % 8) return RT_E_ALIGN;
    a.B[t] = (const bf16_t*)x.B;
    a.At[t] = (const bf16_t*)x.At;
    a.ldb[t] = x.ldb;
    a.lda[t] = x.lda;
    a.nj[t] = x.r_pad / 32;
    a.scale[t] = x.scale;
  }
  a.W0 = (const bf16_t*)W0;
  a.W = (bf16_t*)W;
  a.ld0 = ld0;
  a.ldw = ldw;
  a.N = N;
  a.K = K;
  a.nterms = nterms;
  const dim3 grid((K + kTileK - 1) / kTileK, (N + kTileN - 1) / kTileN), block(256);
  hipLaunchKernelGGL(lora_merge_kernel, grid, block, 0, (hipStream_t)stream, a);
  return rt_hip_status();
}
