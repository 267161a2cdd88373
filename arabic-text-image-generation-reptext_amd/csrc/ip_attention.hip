// rt_ip_attention — o (+)= ip_scale · softmax(bf16(rmsnorm(q)·wq) · Kᵀ · sm_scale) · V: the IP-Adapter term of a double block.
// rt_ip_attention_gated — the same body with an optional fp32 column gate multiplied into ip_scale · acc before the write or
// accumulate (GATED instantiations; the ungated ones are the code rt_ip_attention has always run): the InstantX form, whose term of a
// double block goes through the adaLN gate_msa straight onto the residual rows, and whose single blocks query with all S rows.
// rt_ip_attention_rows — the same body with an fp32 weight per query row (ROWS instantiations; the others are the code they were):
// a regional image prompt. The weight joins ip_scale in fp32; a row of weight 0 is selected out, not multiplied (accumulate: its
// output is neither read nor written; write: +0; its q row never reaches an output), a 16-row tile of such rows reads no q and runs
// no MFMA, and a workgroup of such rows does not stage K / Vᵀ.
//
// Rectangular attention of many query rows (N image tokens) against a handful of image-prompt keys (1 <= n_ip <= 128), one pass,
// no online softmax. Bound by memory: q is read once and o written once; K and V of a head (<= 64 KiB) are staged in LDS once per
// workgroup, which then walks 64·TILES query rows (4 waves x TILES tiles of 16 rows; 256 rows for more than 96 keys, else 128), so
// their re-read (from L2) stays below the q read. The raw q rows of a wave's NEXT tile are loaded before the current tile is computed,
// so that the tiles of a wave are not one serial load -> compute -> store chain; measured alone this was neutral, it is
// kept because it costs 16 registers and no occupancy.
//
// Per 16-row tile a wave computes, on v_mfma_f32_16x16x32_bf16 with fp32 scores, statistics and accumulators:
//   Sᵀ[key][row] = K · Q̂ᵀ     A = K rows from LDS (16 B per lane), B = Q̂: lane (r = l & 15, g = l >> 4) holds columns 32s + 8g .. +7
//                              of query row r, straight from global memory (16 B per lane), RMS-normalised in fp32 and rounded to bf16
//   Oᵀ[d][row]   = Vᵀ · Pᵀ     B = P: the score accumulators of the lane ARE its B fragment (a lane of Sᵀ holds keys 16t + 4g + e of
//                              query row r; k-step u takes tiles 2u and 2u + 1, i.e. keys 32u + 4g + {0..3} and 32u + 16 + 4g + {0..3}),
//                              A = Vᵀ from an LDS image stored key-contiguous, read in that same key order (two 8-byte reads).
// The rows of the Vᵀ tiles are permuted (tile c, row m -> d = 32(c >> 1) + 8(m >> 2) + 4(c & 1) + (m & 3)) so that a lane ends up
// with 8 consecutive output columns of its query row per tile pair: o is written (and, with accumulate, read) 16 bytes per lane.
// The LDS image of Vᵀ is stored in that tile order (row 16c + m), so the 16 lanes of a tile read 16 consecutive rows.
// Keys are padded inside the kernel to KB·32: padded K and V rows are zero in LDS and their scores are masked to -inf.
#include "rt_common.h"

namespace {

constexpr int kKLd = 128 + 8;   // K row stride in LDS (elements): +16 B keeps the 16-byte row reads off one bank

struct IpArgs {
  const bf16_t* q;
  const bf16_t* wq;
  const bf16_t* k;
  const bf16_t* v;
  void* o;
  const float* gate;           // GATED only: [B][>= H·128] fp32, batch stride stride_gb
  int64_t stride_gb;
  int64_t ldq, stride_qb, ldkv, stride_kvb, ldo, stride_ob;
  int32_t N, n_ip, o_f32, accumulate;
  float sm_scale_log2, ip_scale, eps;
  // ROWS only, last so that the other instantiations read their arguments where they always have
  const float* row_w;          // [B or 1][N] fp32 weight per query row, batch stride stride_wb (0: one table)
  int64_t stride_wb;
};

// key blocks of 32; 16-row tiles per wave; an fp32 gate per output column; an fp32 weight per query row (rt_ip_attention_rows)
template <int KB, int TILES, bool GATED, bool ROWS>
__global__ __launch_bounds__(256) void ip_attention_kernel(const IpArgs a) {
  // Vᵀ row stride (elements): NP + 8 puts the 16 rows x 2 lane groups of a half-wave's 8-byte reads on 64 distinct banks
  constexpr int NP = KB * 32, VLD = NP + 8;
  __shared__ __attribute__((aligned(16))) bf16_t Ks[NP * kKLd];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[128 * VLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.x, b = blockIdx.z;        // heads fastest: the workgroups in flight together read neighbouring segments of the same rows
  const int r = lane & 15, g = lane >> 4;

  // ROWS: lane (r, g) holds the weight of row r of the wave's tile g (g < TILES; rows beyond N count as zero). The ballot is the
  // wave's tile mask, bits 16·it .. +15 = the rows of tile `it` that are worth something: wave-uniform, so every skip below is a
  // scalar branch. A workgroup without one such row leaves before K / Vᵀ are staged: the decision comes out of the barrier itself, so
  // all four waves take it together and none waits at the barrier below for a wave that has left.
  float wlane = 0.f;
  unsigned long long wmask = ~0ull;
  auto zero_row = [&](int row) {                  // write mode: a row worth nothing is +0, whatever its q row holds
    if (a.o_f32) {
      f32x4* p = reinterpret_cast<f32x4*>((float*)a.o + (int64_t)b * a.stride_ob + (int64_t)row * a.ldo + h * 128 + 8 * g);
#pragma unroll
      for (int c = 0; c < 8; ++c) p[8 * (c >> 1) + (c & 1)] = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
      u32x4* p = reinterpret_cast<u32x4*>((bf16_t*)a.o + (int64_t)b * a.stride_ob + (int64_t)row * a.ldo + h * 128 + 8 * g);
#pragma unroll
      for (int cp = 0; cp < 4; ++cp) p[4 * cp] = u32x4{0u, 0u, 0u, 0u};
    }
  };
  if constexpr (ROWS) {
    const int wrow = blockIdx.y * (64 * TILES) + g * 64 + wave * 16 + r;
    if (g < TILES && wrow < a.N) wlane = a.row_w[(int64_t)b * a.stride_wb + wrow];
    wmask = __ballot(wlane != 0.f);
    if (!__syncthreads_or(wmask != 0ull)) {       // workgroup-uniform
      if (!a.accumulate && g < TILES && wrow < a.N) {
        // the 4 lanes (r, 0..3) of a row write its 128 columns; here lane (r, g) owns row r of tile g, so it writes all four parts
#pragma unroll 1
        for (int gg = 0; gg < 4; ++gg) {
          if (a.o_f32) {
            f32x4* p = reinterpret_cast<f32x4*>((float*)a.o + (int64_t)b * a.stride_ob + (int64_t)wrow * a.ldo + h * 128 + 32 * gg);
#pragma unroll
            for (int c = 0; c < 8; ++c) p[c] = f32x4{0.f, 0.f, 0.f, 0.f};
          } else {
            u32x4* p = reinterpret_cast<u32x4*>((bf16_t*)a.o + (int64_t)b * a.stride_ob + (int64_t)wrow * a.ldo + h * 128 + 32 * gg);
#pragma unroll
            for (int c = 0; c < 4; ++c) p[c] = u32x4{0u, 0u, 0u, 0u};
          }
        }
      }
      return;
    }
  }
  auto tile_on = [&](int it) { return !ROWS || ((wmask >> (16 * it)) & 0xffffull) != 0ull; };

  // ---- stage K (row-major) and Vᵀ (key-contiguous) of this (batch, head); rows >= n_ip are zero
  {
    const bf16_t* kb = a.k + (int64_t)b * a.stride_kvb + h * 128;
    const bf16_t* vb = a.v + (int64_t)b * a.stride_kvb + h * 128;
    // NP·16 chunks of 16 bytes, 2·KB per thread: every load is issued before the first LDS write (one round trip, not 2·KB)
    u32x4 kreg[2 * KB], vreg[2 * KB];
#pragma unroll
    for (int i = 0; i < 2 * KB; ++i) {
      const int c = tid + 256 * i, key = c >> 4, c8 = (c & 15) * 8;
      kreg[i] = u32x4{0u, 0u, 0u, 0u};
      vreg[i] = u32x4{0u, 0u, 0u, 0u};
      if (key < a.n_ip) {
        kreg[i] = *reinterpret_cast<const u32x4*>(kb + (int64_t)key * a.ldkv + c8);
        vreg[i] = *reinterpret_cast<const u32x4*>(vb + (int64_t)key * a.ldkv + c8);
      }
    }
#pragma unroll
    for (int i = 0; i < 2 * KB; ++i) {
      const int c = tid + 256 * i, key = c >> 4, c8 = (c & 15) * 8;
      const u32x4 kk = kreg[i], vv = vreg[i];
      *reinterpret_cast<u32x4*>(&Ks[key * kKLd + c8]) = kk;
      // column d of V is row 16c + m of the image, (c, m) = the Vᵀ tile and tile row that hold d (see the header)
      const int vr0 = 16 * (2 * (c8 >> 5) + ((c8 >> 2) & 1)) + 4 * ((c8 >> 3) & 3);
#pragma unroll
      for (int e = 0; e < 4; ++e) {      // columns c8 + 2e, c8 + 2e + 1: c8 % 8 == 0, so d & 3 = 2e (& 3), and bit 2 of d is e >> 1
        const int row = vr0 + 16 * (e >> 1) + 2 * (e & 1);
        Vt[row * VLD + key] = (bf16_t)(vv[e] & 0xffffu);
        Vt[(row + 1) * VLD + key] = (bf16_t)(vv[e] >> 16);
      }
    }
  }
  // norm_q.weight of the lane's 32 query columns (32s + 8g + j), fp32
  float wqf[4][8];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(a.wq + 32 * s + 8 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      wqf[s][2 * e] = bf16lo(w[e]);
      wqf[s][2 * e + 1] = bf16hi(w[e]);
    }
  }

  const int row_wg = blockIdx.y * (64 * TILES);
  const bf16_t* qb = a.q + (int64_t)b * a.stride_qb + h * 128 + 8 * g;
  // raw q of the lane's row in tile `it` (rows beyond N read row N - 1: always inside the buffer)
  auto load_q = [&](int it, u32x4 (&dst)[4]) {
    const bf16_t* qr = qb + (int64_t)min(row_wg + it * 64 + wave * 16 + r, a.N - 1) * a.ldq;
#pragma unroll
    for (int s = 0; s < 4; ++s) dst[s] = *reinterpret_cast<const u32x4*>(qr + 32 * s);
  };
  // the lane's output columns are h·128 + 32cp + 8g + 0..7, cp = 0..3: their gate values are read per tile (L1/L2 hits; 12 KiB per
  // batch entry) instead of held in 32 more registers
  const float* grow = GATED ? a.gate + (int64_t)b * a.stride_gb + h * 128 + 8 * g : nullptr;
  u32x4 qnext[4];
  if (tile_on(0)) load_q(0, qnext);
  __syncthreads();                                // K / Vᵀ staged (the q loads above are already in flight)

#pragma unroll 1
  for (int it = 0; it < TILES; ++it) {
    const int row0 = row_wg + it * 64 + wave * 16;
    if (row0 >= a.N) break;                       // wave-uniform; no barrier below
    const int row = row0 + r;
    const bool valid = row < a.N;
    if (!tile_on(it)) {                           // wave-uniform: no q, no RMSNorm, no MFMA; write mode leaves the zeros
      if (it + 1 < TILES && tile_on(it + 1)) load_q(it + 1, qnext);       // the next tile still finds its rows in flight
      if (!a.accumulate && valid) zero_row(row);
      continue;
    }
    u32x4 qraw[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qraw[s] = qnext[s];
    if (it + 1 < TILES && tile_on(it + 1)) load_q(it + 1, qnext);   // a tile worth nothing is not read

    // RMSNorm over the 128 columns of the row: 32 in this lane, the rest in lanes l ^ 16, l ^ 32, l ^ 48
    float qf[4][8], ss = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        qf[s][2 * e] = bf16lo(qraw[s][e]);
        qf[s][2 * e + 1] = bf16hi(qraw[s][e]);
        ss = __builtin_fmaf(qf[s][2 * e], qf[s][2 * e], ss);
        ss = __builtin_fmaf(qf[s][2 * e + 1], qf[s][2 * e + 1], ss);
      }
    ss += __shfl_xor(ss, 16);
    ss += __shfl_xor(ss, 32);
    const float rs = rsqrtf(ss * (1.0f / 128.0f) + a.eps);
    bf16x8 qfrag[4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) qfrag[s][j] = (__bf16)(qf[s][j] * rs * wqf[s][j]);

    // Sᵀ tiles: st[t][e] = score of key 16t + 4g + e for query row r
    f32x4 st[2 * KB];
#pragma unroll
    for (int t = 0; t < 2 * KB; ++t) {
      st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&Ks[(16 * t + r) * kKLd + 32 * s + 8 * g]);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qfrag[s], st[t], 0, 0, 0);
      }
    }
    // softmax over the keys of the row: registers, then the four lane groups
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2 * KB; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (16 * t + 4 * g + e >= a.n_ip) st[t][e] = -INFINITY;
        m = fmaxf(m, st[t][e]);
      }
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));      // finite: key 0 is never masked
    float sum = 0.f;
    bf16x8 pfrag[KB];
#pragma unroll
    for (int t = 0; t < 2 * KB; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = __builtin_amdgcn_exp2f((st[t][e] - m) * a.sm_scale_log2);
        sum += p;
        pfrag[t >> 1][4 * (t & 1) + e] = (__bf16)p;
      }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    // ROWS: the row's weight joins ip_scale in fp32, before the gate and any rounding (w = 1 keeps the bits of the unweighted launch)
    const float wr = ROWS ? __shfl(wlane, 16 * it + r) : 1.0f;
    const float inv = (ROWS ? a.ip_scale * wr : a.ip_scale) / sum;

    // Oᵀ tiles: ot[c][e] = o[row r][d = 32(c >> 1) + 8g + 4(c & 1) + e]
    f32x4 ot[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      ot[c] = f32x4{0.f, 0.f, 0.f, 0.f};
      const bf16_t* vr = &Vt[(16 * c + r) * VLD + 4 * g];
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        const u32x2 lo = *reinterpret_cast<const u32x2*>(vr + 32 * u);
        const u32x2 hi = *reinterpret_cast<const u32x2*>(vr + 32 * u + 16);
        const u32x4 vv = u32x4{lo[0], lo[1], hi[0], hi[1]};
        ot[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vv), pfrag[u], ot[c], 0, 0, 0);
      }
    }
    if (!valid) continue;
    if (ROWS && wr == 0.f) {                      // select, not multiply: accumulate leaves the row's bytes alone, write stores +0
      if (!a.accumulate) zero_row(row);
      continue;
    }
    if (a.o_f32) {
      float* orow = (float*)a.o + (int64_t)b * a.stride_ob + (int64_t)row * a.ldo + h * 128 + 8 * g;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        f32x4* p = reinterpret_cast<f32x4*>(orow + 32 * (c >> 1) + 4 * (c & 1));
        f32x4 x = ot[c] * inv;
        if (GATED) x *= *reinterpret_cast<const f32x4*>(grow + 32 * (c >> 1) + 4 * (c & 1));
        if (a.accumulate) x += *p;
        *p = x;
      }
    } else {
      bf16_t* orow = (bf16_t*)a.o + (int64_t)b * a.stride_ob + (int64_t)row * a.ldo + h * 128 + 8 * g;
#pragma unroll
      for (int cp = 0; cp < 4; ++cp) {
        u32x4* p = reinterpret_cast<u32x4*>(orow + 32 * cp);
        float x[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          x[e] = ot[2 * cp][e] * inv;
          x[4 + e] = ot[2 * cp + 1][e] * inv;
        }
        if (GATED) {
          const f32x4 g0 = *reinterpret_cast<const f32x4*>(grow + 32 * cp), g1 = *reinterpret_cast<const f32x4*>(grow + 32 * cp + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            x[e] *= g0[e];
            x[4 + e] *= g1[e];
          }
        }
        if (a.accumulate) {
          const u32x4 old = *p;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            x[2 * e] += bf16lo(old[e]);
            x[2 * e + 1] += bf16hi(old[e]);
          }
        }
        *p = u32x4{pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3]), pack_bf16x2(x[4], x[5]), pack_bf16x2(x[6], x[7])};
      }
    }
  }
}

template <bool GATED, bool ROWS>
void launch_ip(const IpArgs& a, int B, int H, hipStream_t st) {
  const int kb = (a.n_ip + 31) / 32, rows_per_wg = kb == 4 ? 256 : 128;
  const dim3 grid(H, (a.N + rows_per_wg - 1) / rows_per_wg, B), block(256);
  switch (kb) {
    case 1: hipLaunchKernelGGL((ip_attention_kernel<1, 2, GATED, ROWS>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((ip_attention_kernel<2, 2, GATED, ROWS>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((ip_attention_kernel<3, 2, GATED, ROWS>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((ip_attention_kernel<4, 4, GATED, ROWS>), grid, block, 0, st, a); break;
  }
}

// the one host body: row_w == nullptr is rt_ip_attention_gated (the instantiations without ROWS)
int ip_run(const void* q, int64_t ldq, int64_t stride_qb, const void* wq, const void* k, const void* v, int64_t ldkv, int64_t stride_kvb,
           const float* gate, int64_t stride_gb, const float* row_w, int64_t stride_wb, void* o, int64_t ldo, int64_t stride_ob,
           int32_t o_f32, int32_t accumulate, int32_t B, int32_t N, int32_t H, int32_t n_ip, float sm_scale, float ip_scale, float eps,
           void* stream) {
  if (!q || !wq || !k || !v || !o || B < 1 || N < 1 || H < 1 || n_ip < 1) return RT_E_BADARG;
  if (!(sm_scale > 0.0f)) return RT_E_BADARG;     // the row maximum is taken before the scale is applied
  if (n_ip > 128 || (N + 127) / 128 > 65535 || B > 65535) return RT_E_SHAPE;
  const int64_t d = (int64_t)H * 128;
  if (ldq < d || ldkv < d || ldo < d || stride_qb < 0 || stride_kvb < 0 || stride_ob < 0 || (gate && stride_gb < 0)) return RT_E_BADARG;
  const int o_align = o_f32 ? 4 : 8;     // elements per 16 bytes
  if (!RT_ALIGNED(q, 16) || !RT_ALIGNED(wq, 16) || !RT_ALIGNED(k, 16) || !RT_ALIGNED(v, 16) || !RT_ALIGNED(o, 16) || ldq % 8 ||
      stride_qb % 8 || ldkv % 8 || stride_kvb % 8 || ldo % o_align || stride_ob % o_align || (gate && (!RT_ALIGNED(gate, 16) || stride_gb % 4)))
    return RT_E_ALIGN;
  IpArgs a;
  a.q = (const bf16_t*)q;
  a.wq = (const bf16_t*)wq;
  a.k = (const bf16_t*)k;
  a.v = (const bf16_t*)v;
  a.o = o;
  a.gate = gate;
  a.stride_gb = gate ? stride_gb : 0;
  a.row_w = row_w;
  a.stride_wb = row_w ? stride_wb : 0;
  a.ldq = ldq;
  a.stride_qb = stride_qb;
  a.ldkv = ldkv;
  a.stride_kvb = stride_kvb;
  a.ldo = ldo;
  a.stride_ob = stride_ob;
  a.N = N;
  a.n_ip = n_ip;
  a.o_f32 = o_f32 ? 1 : 0;
  a.accumulate = accumulate ? 1 : 0;
  a.sm_scale_log2 = sm_scale * 1.4426950408889634f;
  a.ip_scale = ip_scale;
  a.eps = eps;
  if (row_w) {
    if (gate) launch_ip<true, true>(a, B, H, (hipStream_t)stream);
    else launch_ip<false, true>(a, B, H, (hipStream_t)stream);
  } else {
    if (gate) launch_ip<true, false>(a, B, H, (hipStream_t)stream);
    else launch_ip<false, false>(a, B, H, (hipStream_t)stream);
  }
  return rt_hip_status();
}

}  // namespace

extern "C" int rt_ip_attention_gated(const void* q, int64_t ldq, int64_t stride_qb, const void* wq, const void* k, const void* v,
                                     int64_t ldkv, int64_t stride_kvb, const float* gate, int64_t stride_gb, void* o, int64_t ldo,
                                     int64_t stride_ob, int32_t o_f32, int32_t accumulate, int32_t B, int32_t N, int32_t H, int32_t n_ip,
                                     float sm_scale, float ip_scale, float eps, void* stream) {
  return ip_run(q, ldq, stride_qb, wq, k, v, ldkv, stride_kvb, gate, stride_gb, nullptr, 0, o, ldo, stride_ob, o_f32, accumulate, B, N, H,
                n_ip, sm_scale, ip_scale, eps, stream);
}

extern "C" int rt_ip_attention_rows(const void* q, int64_t ldq, int64_t stride_qb, const void* wq, const void* k, const void* v,
                                    int64_t ldkv, int64_t stride_kvb, const float* gate, int64_t stride_gb, const float* row_w,
                                    int64_t stride_wb, void* o, int64_t ldo, int64_t stride_ob, int32_t o_f32, int32_t accumulate,
                                    int32_t B, int32_t N, int32_t H, int32_t n_ip, float sm_scale, float ip_scale, float eps, void* stream) {
  if (!row_w || stride_wb < 0) return RT_E_BADARG;     // no weights: rt_ip_attention_gated
  if (!RT_ALIGNED(row_w, 4)) return RT_E_ALIGN;
  return ip_run(q, ldq, stride_qb, wq, k, v, ldkv, stride_kvb, gate, stride_gb, row_w, stride_wb, o, ldo, stride_ob, o_f32, accumulate, B, N,
                H, n_ip, sm_scale, ip_scale, eps, stream);
}

extern "C" int rt_ip_attention(const void* q, int64_t ldq, int64_t stride_qb, const void* wq, const void* k, const void* v,
                               int64_t ldkv, int64_t stride_kvb, void* o, int64_t ldo, int64_t stride_ob, int32_t o_f32,
                               int32_t accumulate, int32_t B, int32_t N, int32_t H, int32_t n_ip, float sm_scale, float ip_scale,
                               float eps, void* stream) {
  return rt_ip_attention_gated(q, ldq, stride_qb, wq, k, v, ldkv, stride_kvb, nullptr, 0, o, ldo, stride_ob, o_f32, accumulate, B, N, H,
                               n_ip, sm_scale, ip_scale, eps, stream);
}
