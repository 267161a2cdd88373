// rt_attention_hd64, rt_attention_hd72 — o = softmax(scale · q kᵀ) v for heads of 64 and of 72, non-causal, no bias: the attention
// of the two vision encoders (image_encoder.py), one launch per layer instead of the per-(batch, head) GEMM ->
// rt_softmax_rows_bias -> rt_transpose_bf16 -> GEMM chain of text_encoders._attention_heads. One kernel template <HD, NW> serves
// both; the two entry points are thin wrappers over one host function.
//   64: CLIP ViT-L/14, 16 heads, 257 tokens, self-attention on the fused q|k|v buffer (q and k/v share strides and row count).
//   72: SigLIP-so400m, 1152 = 16 heads x 72, 729 tokens. Separate query and key counts and strides: one entry point serves the
//       self-attention of its layers (Sq = Sk = 729) and its attention-pooling head (Sq = 1, one probe row shared by the batch:
//       stride_qb = 0, Sk = 729).
//
// Online softmax over key tiles of 64, not one pass with every key of a head in LDS: the one-pass form needs 2·S·64 bf16 (+ padding)
// per workgroup — 66 KiB at S = 257, two workgroups per CU at most, and past the 160 KiB of a CU from S ≈ 600 on, so the bounds
// the entry points have to serve cannot be met by it — while a 64-key tile is 17 KiB (20 KiB for 72) whatever S is, and the rescale
// it costs (one exp2 and 16 multiplies per lane and tile) is small beside the tile's 64 exp2. Upper bounds, set by what is tested,
// not by the kernel: S <= RT_ATTENTION_HD64_MAX_S (4096); Sq, Sk <= RT_ATTENTION_HD72_MAX_S (1024; 729 is tested); B, H <= 65535 (grid).
//
// A workgroup is NW waves; a wave owns 16 query rows for the whole key loop (scores, statistics and O never leave its registers).
// Per key tile the workgroup stages K (row-major) and Vᵀ (key-contiguous) of its (batch, head) in LDS — the loads of tile j + 1 are
// issued before tile j is computed and land in registers, one buffer in LDS, two barriers per tile — and every wave computes, on
// v_mfma_f32_16x16x32_bf16 with fp32 scores, statistics and accumulators, ip_attention.hip's two products:
//   Sᵀ[key][row] = K · Qᵀ      A = K rows from LDS (16 B per lane), B = Q: lane (r = l & 15, g = l >> 4) holds columns 32s + 8g .. +7 of
//                              query row r, read once from global memory (rows past Sq read row Sq - 1 and are not stored)
//   Oᵀ[d][row]  += Vᵀ · Pᵀ     B = P: the lane's score accumulators, exponentiated against the running maximum and rounded to bf16,
//                              ARE its B fragment (keys 32u + 4g + {0..3} and 32u + 16 + 4g + {0..3} of k-step u); A = Vᵀ read in that
//                              key order (two 8-byte reads). The rows of the Vᵀ image are permuted as in ip_attention.hip (tile c, row m
//                              -> d = 32(c >> 1) + 8(m >> 2) + 4(c & 1) + (m & 3)), so a lane ends with 8 consecutive columns per tile
//                              pair: 16-byte stores at columns 32cp + 8g.
// Both statistics of a query row live on the lanes that hold it (r, all four g): a tile's maximum and sum are reduced with two
// shuffles, the accumulators of a lane all belong to its one row, so the rescale is a per-lane scalar. The row sum is taken from
// the unrounded fp32 P; o is normalised once, after the last tile. Keys >= Sk are never loaded: zero rows in LDS, scores masked to
// -inf (key 64j of tile j always exists, so a tile's maximum is finite). The maximum is taken on the raw scores (scale > 0).
//
// LDS images (banking: a ds_read_b128 is served in four groups of 16 lanes, {0-3, 12-15, 20-27}, ..., over 64 banks = sixteen 16-byte
// slots; a ds_read_b64 in two halves of 32 lanes over the same 64 banks).
//   K    64 rows of 128 B, 16-byte chunk c of row k at chunk c ^ (k & 7): the four 16-lane groups of a ds_read_b128 then each cover
//        the 16 slots of a 256-B bank row once (a +16 B row pad leaves them 2-way).
//   Vᵀ   HD rows of 64 + 8 keys: 36-dword rows put the 16 rows x 2 lane groups of a half-wave's 8-byte reads on 64 distinct banks
//        (36 r mod 64 runs over the 16 multiples of 4; g adds 0 or 2, the read is 2 dwords). The 2-byte transposing writes of Vᵀ are
//        not conflict-free (ip_attention.hip's staging); they are paid once per tile and workgroup.
// Not measured with counters yet: the degrees above, and those of the 72 tail below, are derived from the banking rule, not from
// SQ_LDS_BANK_CONFLICT.
//
// What 72 = 2·32 + 8 changes (everything under `if constexpr (HD == 72)`; the head-64 instantiation has none of it):
//   Sᵀ = K · Qᵀ      a third k-step for columns 64..71. A 16x16x32 step feeds 8 columns per lane group, so in the third step only
//                    g = 0 holds real columns; groups 1..3 hold ZEROS in both operands (selected in registers: neither the next
//                    head's columns nor whatever lies behind the last head is ever read, and no 0 x garbage product exists).
//                    Chosen over v_mfma_f32_16x16x16_bf16 for the tail: that instruction takes 4 columns per lane group, so groups
//                    2 and 3 would hold zeros just the same, and q and the K tail would need a second fragment layout (8-byte
//                    reads). It would halve the third step's MFMA time: one of 22 MFMAs per tile and wave, 12 + 10, becomes a half —
//                    about 2 % of the issue slots of a kernel that is bound by the latency of its staging chain, not by the matrix
//                    unit. One MFMA shape and one layout were worth more.
//   Oᵀ += Vᵀ · Pᵀ    72 output columns are 4.5 tiles of 16. Tiles 0..3 are as above; tile 4 holds column 64 + m in row m (not
//                    permuted), so lane groups g = 0, 1 end with columns 64 + 4g .. +3 (one 8-byte store each, 144 B per head keeps
//                    it aligned). Rows 8..15 of tile 4 are rows 72..79 of the Vᵀ image: zeroed once when the kernel starts and
//                    never written, so the fifth tile's A fragment comes from LDS alone — nothing is read from memory beyond the
//                    head — and its accumulator rows 8..15 (groups g = 2, 3) are zeros that are not stored.
//   K in LDS         a row is 9 chunks of 16 B. Chunks 0..7 are kept exactly as above and chunk 8 of every row goes to a SEPARATE
//                    array of 64 x 16 B indexed by the key. The third k-step reads chunk 8 of row 16t + r on all four lane groups
//                    (same address for the four g of a row: a broadcast), and the 16 rows of a group sit on 16 consecutive slots:
//                    conflict-free too. Plain 9-chunk rows (144 B apart, slot = (9k + c) mod 16) were worked out first: a 16-lane
//                    group reads chunk c on eight of its rows and c + 1 on the other eight, and seven of those sixteen slots then
//                    coincide (2-way). Splitting the tail off keeps every read at degree 1 and the staging of chunks 0..7 unchanged.
//   Staging          a tile is 64 keys x 9 chunks for K and for V. Chunks 0..7 are spread over the workgroup (512 / T per thread);
//                    the 64 tail chunks are loaded and stored by the first wave, one key per lane.
//
// Grid: (H, ceil(Sq / 16·NW), B). The key loop is short (5 tiles at S = 257) and a launch this small is bound by the latency of one
// workgroup's chain, not by throughput: NW = 4 is 80 workgroups for ViT-L/14 at B = 1, 16·5, on 256 CUs, and each stages every key
// once for 64 rows; NW = 1 is 272, one wave per workgroup, every CU busy, each staging every key for 16 rows. The LDS writes and the
// MFMAs a CU issues per tile are the same either way (one workgroup's staging, 16 MFMAs per SIMD), so the rule is, on the QUERY
// rows: the largest NW of {4, 2, 1} that still gives one workgroup per CU (256), else NW = 1. so400m at B = 1 runs NW = 2 (368
// workgroups), at B = 4 NW = 4 (768). The pooling call is 16·B one-wave workgroups with one live row walking 12 key tiles:
// latency-bound and tiny, so there is no key split. RT_HD64_WAVES / RT_HD72_WAVES = 1 | 2 | 4 force NW for their head dim (A/B and
// the test that every choice gives the same bits; read on every call, so a process can switch them; the measured times are in
// DESIGN.md §3). A row's arithmetic does not depend on NW: every choice gives the same bits.
#include <stdlib.h>

#include "rt_common.h"

namespace {

constexpr int kVLd = 64 + 8;    // Vᵀ row stride in LDS (elements)

struct SmallHeadArgs {
  const bf16_t* q;
  const bf16_t* k;
  const bf16_t* v;
  bf16_t* o;
  int64_t ldq, stride_qb, ldkv, stride_kvb, ldo, stride_ob;
  int32_t Sq, Sk;
  float scale_log2;
};

template <int HD, int NW>   // head dim; waves per workgroup = 16-row query tiles per workgroup
__global__ __launch_bounds__(64 * NW) void attention_small_head_kernel(const SmallHeadArgs a) {
  static_assert(HD % 8 == 0 && (HD == 64 || HD == 72), "built and tested for heads of 64 and 72 only");
  constexpr bool kTail = HD == 72;                 // chunk 8 of a row: the third k-step and the fifth O tile
  constexpr int kOT = (HD + 15) / 16;              // 16-row tiles of Oᵀ: 4, or 5 with rows 72..79 of the Vᵀ image kept zero
  constexpr int kVRows = 16 * kOT;
  constexpr int T = 64 * NW, CH = 512 / T;         // threads; 16-byte chunks 0..7 per thread, operand and key tile (64 keys x 8 chunks)
  __shared__ __attribute__((aligned(16))) bf16_t Ks[64 * 64];                    // chunks 0..7, swizzled
  __shared__ __attribute__((aligned(16))) bf16_t Kt[kTail ? 64 * 8 : 8];         // chunk 8 of every key (72 only; unused, so not allocated, for 64)
  __shared__ __attribute__((aligned(16))) bf16_t Vt[kVRows * kVLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.x, b = blockIdx.z;
  const int r = lane & 15, g = lane >> 4;
  const bf16_t* kb = a.k + (int64_t)b * a.stride_kvb + h * HD;
  const bf16_t* vb = a.v + (int64_t)b * a.stride_kvb + h * HD;

  if constexpr (kTail)   // rows 72..79 of the Vᵀ image: the unused half of the fifth tile. Published by the first barrier of the key loop.
    for (int i = tid; i < 8 * kVLd / 2; i += T) reinterpret_cast<uint32_t*>(&Vt[HD * kVLd])[i] = 0u;

  u32x4 kreg[CH], vreg[CH], ktail, vtail;
  // chunk c = tid + T·i of a tile: key c >> 3, columns 8(c & 7) .. +7; for 72 the first wave also takes columns 64..71 of key
  // `lane`. Keys >= Sk stay zero.
  auto load_kv = [&](int key0) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = tid + T * i, key = key0 + (c >> 3), c8 = (c & 7) * 8;
      kreg[i] = u32x4{0u, 0u, 0u, 0u};
      vreg[i] = u32x4{0u, 0u, 0u, 0u};
      if (key < a.Sk) {
        kreg[i] = *reinterpret_cast<const u32x4*>(kb + (int64_t)key * a.ldkv + c8);
        vreg[i] = *reinterpret_cast<const u32x4*>(vb + (int64_t)key * a.ldkv + c8);
      }
    }
    if constexpr (kTail)
      if (wave == 0) {
        ktail = u32x4{0u, 0u, 0u, 0u};
        vtail = u32x4{0u, 0u, 0u, 0u};
        if (key0 + lane < a.Sk) {
          ktail = *reinterpret_cast<const u32x4*>(kb + (int64_t)(key0 + lane) * a.ldkv + 64);
          vtail = *reinterpret_cast<const u32x4*>(vb + (int64_t)(key0 + lane) * a.ldkv + 64);
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
    if constexpr (kTail)
      if (wave == 0) {
        *reinterpret_cast<u32x4*>(&Kt[lane * 8]) = ktail;
#pragma unroll
        for (int e = 0; e < 4; ++e) {              // column 64 + 2e (+1) is row 64 + 2e (+1): the fifth tile is not permuted
          Vt[(64 + 2 * e) * kVLd + lane] = (bf16_t)(vtail[e] & 0xffffu);
          Vt[(65 + 2 * e) * kVLd + lane] = (bf16_t)(vtail[e] >> 16);
        }
      }
  };

  const int row0 = (blockIdx.y * NW + wave) * 16;
  const bool active = row0 < a.Sq;                 // wave-uniform; an idle wave still stages and meets the barriers
  const int row = row0 + r;
  bf16x8 qfrag[kTail ? 3 : 2];
  {
    const bf16_t* qr = a.q + (int64_t)b * a.stride_qb + (int64_t)min(row, a.Sq - 1) * a.ldq + h * HD;
#pragma unroll
    for (int s = 0; s < 2; ++s) qfrag[s] = *reinterpret_cast<const bf16x8*>(qr + 32 * s + 8 * g);
    if constexpr (kTail) {
      u32x4 t = u32x4{0u, 0u, 0u, 0u};
      if (g == 0) t = *reinterpret_cast<const u32x4*>(qr + 64);
      qfrag[2] = __builtin_bit_cast(bf16x8, t);
    }
  }

  float m = -INFINITY, l = 0.f;
  // ot[c][e], c < 4 = o[row r][d = 32(c >> 1) + 8g + 4(c & 1) + e]; ot[4][e] = o[row r][64 + 4g + e] for g < 2; not yet normalised
  f32x4 ot[kOT];
#pragma unroll
  for (int c = 0; c < kOT; ++c) ot[c] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nt = (a.Sk + 63) >> 6;
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
      const int kr = 16 * t + r;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&Ks[kr * 64 + 8 * ((4 * s + g) ^ (kr & 7))]);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qfrag[s], st[t], 0, 0, 0);
      }
      if constexpr (kTail) {
        u32x4 kt = *reinterpret_cast<const u32x4*>(&Kt[kr * 8]);   // all four g read the row's tail; only g = 0 keeps it
        if (g != 0) kt = u32x4{0u, 0u, 0u, 0u};
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kt), qfrag[2], st[t], 0, 0, 0);
      }
    }
    float mt = -INFINITY;
    const int key_lane = 64 * j + 4 * g;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (key_lane + 16 * t + e >= a.Sk) st[t][e] = -INFINITY;
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
    for (int c = 0; c < kOT; ++c) {
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
  if (!active || row >= a.Sq) return;
  const float inv = 1.0f / l;
  bf16_t* orow = a.o + (int64_t)b * a.stride_ob + (int64_t)row * a.ldo + h * HD;
#pragma unroll
  for (int cp = 0; cp < 2; ++cp) {
    float x[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x[e] = ot[2 * cp][e] * inv;
      x[4 + e] = ot[2 * cp + 1][e] * inv;
    }
    *reinterpret_cast<u32x4*>(orow + 32 * cp + 8 * g) =
        u32x4{pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3]), pack_bf16x2(x[4], x[5]), pack_bf16x2(x[6], x[7])};
  }
  if constexpr (kTail)
    if (g < 2)                                     // columns 64 + 4g .. +3; groups 2 and 3 hold the zero rows 72..79
      *reinterpret_cast<u32x2*>(orow + 64 + 4 * g) = u32x2{pack_bf16x2(ot[4][0] * inv, ot[4][1] * inv), pack_bf16x2(ot[4][2] * inv, ot[4][3] * inv)};
}

int forced_waves(const char* name) {               // A/B and the bit-equality tests; read per call, so a process can switch it
  const char* e = getenv(name);
  const int v = e ? atoi(e) : 0;
  return (v == 1 || v == 2 || v == 4) ? v : 0;
}

template <int HD>
int attention_small_head(const void* q, int64_t ldq, int64_t stride_qb, const void* k, const void* v, int64_t ldkv, int64_t stride_kvb,
                         void* o, int64_t ldo, int64_t stride_ob, int32_t B, int32_t Sq, int32_t Sk, int32_t H, float scale, int32_t max_s,
                         const char* waves_env, void* stream) {
  if (!q || !k || !v || !o || B < 1 || Sq < 1 || Sk < 1 || H < 1) return RT_E_BADARG;
  if (!(scale > 0.0f)) return RT_E_BADARG;         // the row maximum is taken before the scale is applied
  if (Sq > max_s || Sk > max_s || B > 65535 || H > 65535) return RT_E_SHAPE;
  const int64_t d = (int64_t)H * HD;
  if (ldq < d || ldkv < d || ldo < d || stride_qb < 0 || stride_kvb < 0 || stride_ob < 0) return RT_E_BADARG;
  if (!RT_ALIGNED(q, 16) || !RT_ALIGNED(k, 16) || !RT_ALIGNED(v, 16) || !RT_ALIGNED(o, 16) || ldq % 8 || stride_qb % 8 || ldkv % 8 ||
      stride_kvb % 8 || ldo % 8 || stride_ob % 8)
    return RT_E_ALIGN;
  SmallHeadArgs a;
  a.q = (const bf16_t*)q;
  a.k = (const bf16_t*)k;
  a.v = (const bf16_t*)v;
  a.o = (bf16_t*)o;
  a.ldq = ldq;
  a.stride_qb = stride_qb;
  a.ldkv = ldkv;
  a.stride_kvb = stride_kvb;
  a.ldo = ldo;
  a.stride_ob = stride_ob;
  a.Sq = Sq;
  a.Sk = Sk;
  a.scale_log2 = scale * 1.4426950408889634f;
  auto workgroups = [&](int nw) { return (int64_t)B * H * ((Sq + 16 * nw - 1) / (16 * nw)); };
  int nw = forced_waves(waves_env);
  if (!nw) nw = workgroups(4) >= 256 ? 4 : workgroups(2) >= 256 ? 2 : 1;
  const dim3 grid(H, (Sq + 16 * nw - 1) / (16 * nw), B);
  const hipStream_t st = (hipStream_t)stream;
  switch (nw) {
    case 4: hipLaunchKernelGGL((attention_small_head_kernel<HD, 4>), grid, dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL((attention_small_head_kernel<HD, 2>), grid, dim3(128), 0, st, a); break;
    default: hipLaunchKernelGGL((attention_small_head_kernel<HD, 1>), grid, dim3(64), 0, st, a); break;
  }
  return rt_hip_status();
}

}  // namespace

extern "C" int rt_attention_hd64(const void* q, const void* k, const void* v, int64_t ld, int64_t stride_b, void* o, int64_t ldo,
                                 int64_t stride_ob, int32_t B, int32_t S, int32_t H, float scale, void* stream) {
  return attention_small_head<64>(q, ld, stride_b, k, v, ld, stride_b, o, ldo, stride_ob, B, S, S, H, scale, RT_ATTENTION_HD64_MAX_S,
                                  "RT_HD64_WAVES", stream);
}

extern "C" int rt_attention_hd72(const void* q, int64_t ldq, int64_t stride_qb, const void* k, const void* v, int64_t ldkv,
                                 int64_t stride_kvb, void* o, int64_t ldo, int64_t stride_ob, int32_t B, int32_t Sq, int32_t Sk,
                                 int32_t H, float scale, void* stream) {
  return attention_small_head<72>(q, ldq, stride_qb, k, v, ldkv, stride_kvb, o, ldo, stride_ob, B, Sq, Sk, H, scale,
                                  RT_ATTENTION_HD72_MAX_S, "RT_HD72_WAVES", stream);
}
