// rt_attention_hd64 — o = softmax(scale · q kᵀ) v for heads of 64, non-causal, no bias: the self-attention of the CLIP vision
// encoder (image_encoder.py; ViT-L/14: 16 heads, 257 tokens), one launch per layer instead of the per-(batch, head)
// GEMM -> rt_softmax_rows_bias -> rt_transpose_bf16 -> GEMM chain of text_encoders._attention_heads.
//
// Online softmax over key tiles of 64, not one pass with every key of a head in LDS: the one-pass form needs 2·S·64 bf16 (+ padding)
// per workgroup — 66 KiB at S = 257, two workgroups per CU at most, and past the 160 KiB of a CU from S ≈ 600 on, so the bound of
// 1024 the entry point has to serve cannot be met by it — while a 64-key tile is 17 KiB whatever S is, and the rescale it costs
// (one exp2 and 16 multiplies per lane and tile) is small beside the tile's 64 exp2. Upper bound: S <= RT_ATTENTION_HD64_MAX_S (4096), set by what is
// tested, not by the kernel; B, H <= 65535 (grid).
//
// A workgroup is NW waves; a wave owns 16 query rows for the whole key loop (scores, statistics and O never leave its registers).
// Per key tile the workgroup stages K (row-major) and Vᵀ (key-contiguous) of its (batch, head) in LDS — the loads of tile j + 1 are
// issued before tile j is computed and land in registers, one buffer in LDS, two barriers per tile — and every wave computes, on
// v_mfma_f32_16x16x32_bf16 with fp32 scores, statistics and accumulators, ip_attention.hip's two products:
//   Sᵀ[key][row] = K · Qᵀ      A = K rows from LDS (16 B per lane), B = Q: lane (r = l & 15, g = l >> 4) holds columns 32s + 8g .. +7 of
//                              query row r, read once from global memory (rows past S read row S - 1 and are not stored)
//   Oᵀ[d][row]  += Vᵀ · Pᵀ     B = P: the lane's score accumulators, exponentiated against the running maximum and rounded to bf16,
//                              ARE its B fragment (keys 32u + 4g + {0..3} and 32u + 16 + 4g + {0..3} of k-step u); A = Vᵀ read in that
//                              key order (two 8-byte reads). The rows of the Vᵀ image are permuted as in ip_attention.hip (tile c, row m
//                              -> d = 32(c >> 1) + 8(m >> 2) + 4(c & 1) + (m & 3)), so a lane ends with 8 consecutive columns per tile pair.
// Both statistics of a query row live on the lanes that hold it (r, all four g): a tile's maximum and sum are reduced with two
// shuffles, the accumulators of a lane all belong to its one row, so the rescale is a per-lane scalar. The row sum is taken from
// the unrounded fp32 P; o is normalised once, after the last tile. Keys past S: zero rows in LDS, scores masked to -inf (key 64j of
// tile j always exists, so a tile's maximum is finite). The maximum is taken on the raw scores (scale > 0).
//
// LDS images. K: 64 rows of 128 B, 16-byte chunk c of row k at chunk c ^ (k & 7): the four 16-lane groups of a ds_read_b128
// ({0-3, 12-15, 20-27}, ...) then each cover the 16 slots of a 256-B bank row once (a +16 B row pad leaves them 2-way). Vᵀ: 64 rows of
// 64 + 8 keys: 36-dword rows put the 16 rows x 2 lane groups of a half-wave's 8-byte reads on 64 distinct banks. The 2-byte
// transposing writes of Vᵀ are not conflict-free (ip_attention.hip's staging); they are paid once per tile and workgroup.
//
// Grid: (H, ceil(S / 16·NW), B). The key loop is short (5 tiles at S = 257) and a launch this small is bound by the latency of one
// workgroup's chain, not by throughput: NW = 4 is 80 workgroups for ViT-L/14 at B = 1, 16·5, on 256 CUs, and each stages every key
// once for 64 rows; NW = 1 is 272, one wave per workgroup, every CU busy, each staging every key for 16 rows. The LDS writes and the
// MFMAs a CU issues per tile are the same either way (one workgroup's staging, 16 MFMAs per SIMD), so the rule is: the largest NW
// of {4, 2, 1} that still gives one workgroup per CU (256), else NW = 1. RT_HD64_WAVES = 1 | 2 | 4 forces NW (A/B only; the
// measured times are in DESIGN.md §3). A row's arithmetic does not depend on NW: every choice gives the same bits.
#include <stdlib.h>

#include "rt_common.h"

namespace {

constexpr int kVLd = 64 + 8;    // Vᵀ row stride in LDS (elements)

struct Hd64Args {
  const bf16_t* q;
  const bf16_t* k;
  const bf16_t* v;
  bf16_t* o;
  int64_t ld, stride_b, ldo, stride_ob;
  int32_t S;
  float scale_log2;
};

template <int NW>   // waves per workgroup = 16-row query tiles per workgroup
__global__ __launch_bounds__(64 * NW) void attention_hd64_kernel(const Hd64Args a) {
  constexpr int T = 64 * NW, CH = 512 / T;         // threads; 16-byte chunks per thread, operand and key tile (64 keys x 8 chunks)
  __shared__ __attribute__((aligned(16))) bf16_t Ks[64 * 64];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[64 * kVLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.x, b = blockIdx.z;
  const int r = lane & 15, g = lane >> 4;
  const bf16_t* kb = a.k + (int64_t)b * a.stride_b + h * 64;
  const bf16_t* vb = a.v + (int64_t)b * a.stride_b + h * 64;

  u32x4 kreg[CH], vreg[CH];
  // chunk c = tid + T·i of a tile: key c >> 3, columns 8(c & 7) .. +7; keys >= S stay zero
  auto load_kv = [&](int key0) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = tid + T * i, key = key0 + (c >> 3), c8 = (c & 7) * 8;
      kreg[i] = u32x4{0u, 0u, 0u, 0u};
      vreg[i] = u32x4{0u, 0u, 0u, 0u};
      if (key < a.S) {
        kreg[i] = *reinterpret_cast<const u32x4*>(kb + (int64_t)key * a.ld + c8);
        vreg[i] = *reinterpret_cast<const u32x4*>(vb + (int64_t)key * a.ld + c8);
      }
    }
  };
  auto store_kv = [&]() {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = tid + T * i, key = c >> 3, j = c & 7;
      const u32x4 kk = kreg[i], vv = vreg[i];
      *reinterpret_cast<u32x4*>(&Ks[key * 64 + 8 * (j ^ (key & 7))]) = kk;
      // column d = 8j + 2e (+1) of V is row 16c' + m of the image, (c', m) = the Vᵀ tile and tile row that hold d (see the header)
      const int vr0 = 32 * (j >> 2) + 4 * (j & 3);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = vr0 + 16 * (e >> 1) + 2 * (e & 1);
        Vt[row * kVLd + key] = (bf16_t)(vv[e] & 0xffffu);
        Vt[(row + 1) * kVLd + key] = (bf16_t)(vv[e] >> 16);
      }
    }
  };

  const int row0 = (blockIdx.y * NW + wave) * 16;
  const bool active = row0 < a.S;                  // wave-uniform; an idle wave still stages and meets the barriers
  const int row = row0 + r;
  bf16x8 qfrag[2];
  {
    const bf16_t* qr = a.q + (int64_t)b * a.stride_b + (int64_t)min(row, a.S - 1) * a.ld + h * 64 + 8 * g;
#pragma unroll
    for (int s = 0; s < 2; ++s) qfrag[s] = *reinterpret_cast<const bf16x8*>(qr + 32 * s);
  }

  float m = -INFINITY, l = 0.f;
  f32x4 ot[4];                                     // ot[c][e] = o[row r][d = 32(c >> 1) + 8g + 4(c & 1) + e], not yet normalised
#pragma unroll
  for (int c = 0; c < 4; ++c) ot[c] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nt = (a.S + 63) >> 6;
  load_kv(0);
#pragma unroll 1
  for (int j = 0; j < nt; ++j) {
    if (j) __syncthreads();                        // every wave is done with tile j - 1
    store_kv();
    __syncthreads();
    if (j + 1 < nt) load_kv(64 * (j + 1));         // in flight while this tile is computed
    if (!active) continue;

    // Sᵀ tiles: st[t][e] = score of key 64j + 16t + 4g + e for query row r
    f32x4 st[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int kr = 16 * t + r;
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&Ks[kr * 64 + 8 * ((4 * s + g) ^ (kr & 7))]);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qfrag[s], st[t], 0, 0, 0);
      }
    }
    float mt = -INFINITY;
    const int key_lane = 64 * j + 4 * g;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (key_lane + 16 * t + e >= a.S) st[t][e] = -INFINITY;
        mt = fmaxf(mt, st[t][e]);
      }
    mt = fmaxf(mt, __shfl_xor(mt, 16));
    mt = fmaxf(mt, __shfl_xor(mt, 32));            // finite: key 64j is never masked
    const float mn = fmaxf(m, mt);
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * a.scale_log2);      // first tile: exp2(-inf) = 0
    float ps = 0.f;
    bf16x8 pfrag[2];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = __builtin_amdgcn_exp2f((st[t][e] - mn) * a.scale_log2);
        ps += p;
        pfrag[t >> 1][4 * (t & 1) + e] = (__bf16)p;
      }
    ps += __shfl_xor(ps, 16);
    ps += __shfl_xor(ps, 32);
    l = l * alpha + ps;
    m = mn;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      ot[c] *= alpha;
      const bf16_t* vr = &Vt[(16 * c + r) * kVLd + 4 * g];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const u32x2 lo = *reinterpret_cast<const u32x2*>(vr + 32 * u);
        const u32x2 hi = *reinterpret_cast<const u32x2*>(vr + 32 * u + 16);
        const u32x4 vv = u32x4{lo[0], lo[1], hi[0], hi[1]};
        ot[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vv), pfrag[u], ot[c], 0, 0, 0);
      }
    }
  }
  if (!active || row >= a.S) return;
  const float inv = 1.0f / l;
  bf16_t* orow = a.o + (int64_t)b * a.stride_ob + (int64_t)row * a.ldo + h * 64 + 8 * g;
#pragma unroll
  for (int cp = 0; cp < 2; ++cp) {
    float x[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x[e] = ot[2 * cp][e] * inv;
      x[4 + e] = ot[2 * cp + 1][e] * inv;
    }
    *reinterpret_cast<u32x4*>(orow + 32 * cp) =
        u32x4{pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3]), pack_bf16x2(x[4], x[5]), pack_bf16x2(x[6], x[7])};
  }
}

int forced_waves() {
  static const int nw = [] {
    const char* e = getenv("RT_HD64_WAVES");       // A/B only
    const int v = e ? atoi(e) : 0;
    return (v == 1 || v == 2 || v == 4) ? v : 0;
  }();
  return nw;
}

}  // namespace

extern "C" int rt_attention_hd64(const void* q, const void* k, const void* v, int64_t ld, int64_t stride_b, void* o, int64_t ldo,
                                 int64_t stride_ob, int32_t B, int32_t S, int32_t H, float scale, void* stream) {
  if (!q || !k || !v || !o || B < 1 || S < 1 || H < 1) return RT_E_BADARG;
  if (!(scale > 0.0f)) return RT_E_BADARG;         // the row maximum is taken before the scale is applied
  if (S > RT_ATTENTION_HD64_MAX_S || B > 65535 || H > 65535) return RT_E_SHAPE;
  const int64_t d = (int64_t)H * 64;
  if (ld < d || ldo < d || stride_b < 0 || stride_ob < 0) return RT_E_BADARG;
  if (!RT_ALIGNED(q, 16) || !RT_ALIGNED(k, 16) || !RT_ALIGNED(v, 16) || !RT_ALIGNED(o, 16) || ld % 8 || stride_b % 8 || ldo % 8 ||
      stride_ob % 8)
    return RT_E_ALIGN;
  Hd64Args a;
  a.q = (const bf16_t*)q;
  a.k = (const bf16_t*)k;
  a.v = (const bf16_t*)v;
  a.o = (bf16_t*)o;
  a.ld = ld;
  a.stride_b = stride_b;
  a.ldo = ldo;
  a.stride_ob = stride_ob;
  a.S = S;
  a.scale_log2 = scale * 1.4426950408889634f;
  auto workgroups = [&](int nw) { return (int64_t)B * H * ((S + 16 * nw - 1) / (16 * nw)); };
  int nw = forced_waves();
  if (!nw) nw = workgroups(4) >= 256 ? 4 : workgroups(2) >= 256 ? 2 : 1;
  const dim3 grid(H, (S + 16 * nw - 1) / (16 * nw), B);
  const hipStream_t st = (hipStream_t)stream;
  switch (nw) {
    case 4: hipLaunchKernelGGL((attention_hd64_kernel<4>), grid, dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL((attention_hd64_kernel<2>), grid, dim3(128), 0, st, a); break;
    default: hipLaunchKernelGGL((attention_hd64_kernel<1>), grid, dim3(64), 0, st, a); break;
  }
  return rt_hip_status();
}
