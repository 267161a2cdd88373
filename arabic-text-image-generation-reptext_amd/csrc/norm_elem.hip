// HBM-bound kernels of the denoising path: LayerNorm+modulation, q/k RMSNorm+RoPE, adaLN GEMV,
// timestep/RoPE tables, Euler step, latent pack/unpack, casts. All loads/stores are 8–16 B per lane,
// statistics in fp32. Math per SURVEY.md Appendix A.1/A.2/A.5/A.6 and PIPE:550-570,1109.
#include "rt_common.h"
#include "philox.h"
#include <stdlib.h>
#include <type_traits>

namespace {

// The tail of the per-row e4m3 producers (one wave per row), once the lanes know their maxima: the row's scale, stored by lane 0,
// then every chunk times the reciprocal, clamped, packed and stored as 8 bytes. get(c, col, y) hands over chunk c (columns col .. +7)
// as the kernel kept it; NCH > 0: the lane's chunks are c = 0 .. NCH-1 (unrolled, those inside the row), NCH == 0: it strides the row.
template <int NCH, class Get>
__device__ __forceinline__ void quantize_row_tail(float amax, int lane, int D, float* __restrict__ scale, uint8_t* __restrict__ orow, Get get) {
  const float sc = rt_e4m3_row_scale(wave_max(amax));
  const float inv = 1.f / sc;
  if (lane == 0) *scale = sc;
  auto put = [&](int c, int col) {
    float y[8];
    get(c, col, y);
#pragma unroll
    for (int i = 0; i < 8; ++i) y[i] = rt_sat_e4m3(y[i] * inv);
    *reinterpret_cast<u32x2*>(orow + col) = rt_pack_e4m3x8(y);
  };
  if constexpr (NCH > 0) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int col = (c * 64 + lane) * 8;
      if (col < D) put(c, col);
    }
  } else {
    for (int col = lane * 8; col < D; col += 512) put(0, col);
  }
}

// ---------------------------------------------------------------------------------------------------
// LayerNorm (no affine) + (1+scale)·x + shift. One wave per row, row kept in registers (single HBM read).
// ---------------------------------------------------------------------------------------------------
// A launch covers one or two row segments (rt_layernorm_modulate_pair: image rows + text rows of a double block), each with its own
// tensors, leading dimensions and adaLN vectors; a wave picks its segment from its row index and then works as before.
struct LnLaunch {
  rt_ln_segment seg[2];
  int rows0;            // rows of segment 0; rows >= rows0 belong to segment 1
  int rows;             // all rows
};

template <bool X_F32, int NCH, bool OUT_FP8 = false>   // NCH = chunks of 8 elements per lane  (D <= 64*8*NCH)
__global__ __launch_bounds__(256) void layernorm_mod_kernel(const LnLaunch L, int D, float eps, float* __restrict__ row_scale = nullptr) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= L.rows) return;
  const bool second = row >= L.rows0;                  // wave-uniform
  const rt_ln_segment& sg = L.seg[second ? 1 : 0];
  const void* __restrict__ x = sg.x;
  bf16_t* __restrict__ out = reinterpret_cast<bf16_t*>(sg.out);
  const float* __restrict__ shift = sg.shift;
  const float* __restrict__ scale = sg.scale;
  const int64_t ldx = sg.ldx, stride_xb = sg.stride_xb, ldo = sg.ldo, stride_ob = sg.stride_ob, mod_ld = sg.mod_ld;
  const int rows_per_batch = sg.rows_per_batch;
  const int srow = second ? row - L.rows0 : row;
  const int b = srow / rows_per_batch, r = srow - b * rows_per_batch;
  const void* xrow = rt_row<X_F32>(x, b * stride_xb + (int64_t)r * ldx);
  float v[NCH][8];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * 64 + lane) * 8;
    if (col < D) {
      rt_load8<X_F32>(xrow, col, v[c]);
#pragma unroll
      for (int i = 0; i < 8; ++i) s += v[c][i];
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[c][i] = 0.f;
    }
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * 64 + lane) * 8;
    if (col < D) {
#pragma unroll
      for (int i = 0; i < 8; ++i) { const float d = v[c][i] - mean; q += d * d; }
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
  float amax = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col = (c * 64 + lane) * 8;
    if (col < D) {
      float y[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) y[i] = (v[c][i] - mean) * rstd;
      if (scale) {
        const float* sc = scale + b * mod_ld + col;
        const float* sh = shift + b * mod_ld + col;
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(sc), s1 = *reinterpret_cast<const f32x4*>(sc + 4);
        const f32x4 h0 = *reinterpret_cast<const f32x4*>(sh), h1 = *reinterpret_cast<const f32x4*>(sh + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          y[i] = y[i] * (1.f + s0[i]) + h0[i];
          y[4 + i] = y[4 + i] * (1.f + s1[i]) + h1[i];
        }
      }
      if constexpr (OUT_FP8) {                       // keep the modulated row in registers; quantise after the row max is known
#pragma unroll
        for (int i = 0; i < 8; ++i) { v[c][i] = y[i]; amax = fmaxf(amax, fabsf(y[i])); }
      } else {
        rt_store8(out + b * stride_ob + (int64_t)r * ldo + col, y);
      }
    }
  }
  if constexpr (OUT_FP8)
    quantize_row_tail<NCH>(amax, lane, D, row_scale + row, reinterpret_cast<uint8_t*>(out) + b * stride_ob + (int64_t)r * ldo,
                           [&](int c, int, float (&y)[8]) {
#pragma unroll
                             for (int i = 0; i < 8; ++i) y[i] = v[c][i];
                           });
}

// ---------------------------------------------------------------------------------------------------
// Row-wise e4m3 quantisation (weights once at load; activation rows that do not come out of a LayerNorm).
// One wave per row. bf16 rows of up to 64·8·NCH elements are read ONCE and held packed in registers between the max pass and
// the convert pass (NCH > 0); longer or f32 rows are read twice (NCH == 0).
// ---------------------------------------------------------------------------------------------------
template <bool X_F32, int NCH>
__global__ __launch_bounds__(256) void quantize_rows_fp8_kernel(const void* __restrict__ x, int64_t ldx, uint8_t* __restrict__ out,
                                                                int64_t ldo, float* __restrict__ scale, int rows, int D) {
  static_assert(NCH == 0 || !X_F32, "only bf16 rows are held in registers");
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const void* xrow = rt_row<X_F32>(x, (int64_t)row * ldx);
  u32x4 v[NCH > 0 ? NCH : 1];
  float amax = 0.f;
  if constexpr (NCH > 0) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int col = (c * 64 + lane) * 8;
      v[c] = u32x4{0u, 0u, 0u, 0u};
      if (col < D) v[c] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16_t*>(xrow) + col);
#pragma unroll
      for (int i = 0; i < 4; ++i) amax = fmaxf(amax, fmaxf(fabsf(bf16lo(v[c][i])), fabsf(bf16hi(v[c][i]))));
    }
  } else {
    for (int col = lane * 8; col < D; col += 512) {
      float y[8];
      rt_load8<X_F32>(xrow, col, y);
#pragma unroll
      for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(y[i]));
    }
  }
  quantize_row_tail<NCH>(amax, lane, D, scale + row, out + (int64_t)row * ldo, [&](int c, int col, float (&z)[8]) {
    if constexpr (NCH > 0) rt_unpack8(v[c], z);
    else rt_load8<X_F32>(xrow, col, z);
  });
}

// MX block quantisation (reptext_hip.h: rt_quantize_mx_fp8): 8 elements per thread, 4 threads per 32-element block.
template <bool X_F32>
__global__ __launch_bounds__(256) void quantize_mx_fp8_kernel(const void* __restrict__ x, int64_t ldx, uint8_t* __restrict__ out, int64_t ldo,
                                                              uint8_t* __restrict__ bscale, int64_t plane, int rows, int D) {
  const int per_row = D >> 3;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int row = (int)(idx / per_row);
  const int col = (int)(idx - (int64_t)row * per_row) * 8;
  const bool ok = row < rows;                             // whole 4-lane groups are in or out together (per_row % 32 == 0)
  float y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = 0.f;
  if (ok) rt_load8<X_F32>(rt_row<X_F32>(x, (int64_t)row * ldx), col, y);
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(y[i]));
  amax = fmaxf(amax, __shfl_xor(amax, 1));
  amax = fmaxf(amax, __shfl_xor(amax, 2));
  const int sb = rt_mx_scale_byte(amax);
  const float inv = rt_mx_inv_scale(sb);
  if (!ok) return;
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = rt_sat_e4m3(y[i] * inv);
  *reinterpret_cast<u32x2*>(out + (int64_t)row * ldo + col) = rt_pack_e4m3x8(y);
  if ((threadIdx.x & 3) == 0) bscale[rt_mx_scale_offset(row, col, plane)] = (uint8_t)sb;
}

// ---------------------------------------------------------------------------------------------------
// q/k RMSNorm(128) + RoPE in place. 16 lanes per 128-vector (8 elements = 4 rotation pairs each),
// 4 vectors per wave. Grid covers B*S*H*2 vectors (q and k).
// ---------------------------------------------------------------------------------------------------
// A 16-lane group takes one token row and QK_HC heads of it (q and k: 2·QK_HC vectors of 128), so the row's cos/sin entries and
// the norm weights are loaded once per 2·QK_HC vectors. Measured at 4608×24 heads: one vector per group 21.6 µs, QK_HC = 1 19.7 µs,
// 2: 22.9, 4: 33 — the kernel lives on wave-level parallelism, longer per-lane chains lose more than the table bytes they save.
constexpr int QK_HC = 1;
__global__ __launch_bounds__(256) void qk_rmsnorm_rope_kernel(
    bf16_t* __restrict__ buf, int64_t ld, int64_t stride_b, int64_t q_off, int64_t k_off,
    const bf16_t* __restrict__ wq_txt, const bf16_t* __restrict__ wk_txt, const bf16_t* __restrict__ wq_img,
    const bf16_t* __restrict__ wk_img, const float* __restrict__ cosv, const float* __restrict__ sinv, int B, int S,
    int T, int H, float eps) {
  const int nchunk = (H + QK_HC - 1) / QK_HC;
  const int64_t grp = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);   // (row, head chunk)
  const int sub = threadIdx.x & 15;
  if (grp >= (int64_t)B * S * nchunk) return;   // whole 16-lane groups exit together; shuffles below stay within the group
  const int hc = (int)(grp % nchunk);
  const int64_t row = grp / nchunk;
  const int s = (int)(row % S);
  const int b = (int)(row / S);
  bf16_t* base = buf + b * stride_b + (int64_t)s * ld + sub * 8;
  const rt_qk_row t = rt_qk_load_row(cosv, sinv, wq_txt, wk_txt, wq_img, wk_img, s, T, sub);
  u32x4 u[2 * QK_HC];
#pragma unroll
  for (int v = 0; v < 2 * QK_HC; ++v) {
    const int h = hc * QK_HC + (v >> 1);
    u[v] = u32x4{0u, 0u, 0u, 0u};
    if (h < H) u[v] = *reinterpret_cast<const u32x4*>(base + ((v & 1) ? k_off : q_off) + h * 128);
  }
#pragma unroll
  for (int v = 0; v < 2 * QK_HC; ++v) {
    const int h = hc * QK_HC + (v >> 1);
    const u32x4 o = rt_qk_norm_rope8(u[v], (v & 1) ? t.wk : t.wq, t.cs, t.sn, eps);
    if (h < H) *reinterpret_cast<u32x4*>(base + ((v & 1) ? k_off : q_off) + h * 128) = o;
  }
}

// ---------------------------------------------------------------------------------------------------
// GEMV on fp32 activations, bf16 weights: y[b][n] (+)= post(Σ_k pre(x[b][k]) W[n][k] + bias[n]).
// One wave per output row n; x staged (pre-activated) in LDS as fp32; B <= 8 per launch.
// ---------------------------------------------------------------------------------------------------
constexpr int GEMV_MAXB = 8;
__global__ __launch_bounds__(256) void gemv_bf16w_kernel(const float* __restrict__ x, int64_t ldx,
                                                          const bf16_t* __restrict__ W, int64_t ldw,
                                                          const bf16_t* __restrict__ bias, float* __restrict__ y,
                                                          int64_t ldy, int B, int N, int K, int silu_in, int silu_out,
                                                          int accumulate) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xs = reinterpret_cast<float*>(smem);   // [B][K]
  for (int i = threadIdx.x; i < B * K; i += blockDim.x) {
    const int b = i / K, k = i - b * K;
    float v = x[b * ldx + k];
    xs[i] = silu_in ? silu_f(v) : v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  constexpr int ROWS_PER_WAVE = 4;
  for (int rr = 0; rr < ROWS_PER_WAVE; ++rr) {
    const int n = (blockIdx.x * 4 + wave) * ROWS_PER_WAVE + rr;
    if (n >= N) break;
    float acc[GEMV_MAXB];
#pragma unroll
    for (int b = 0; b < GEMV_MAXB; ++b) acc[b] = 0.f;
    const bf16_t* wr = W + (int64_t)n * ldw;
    for (int k = lane * 8; k < K; k += 512) {
      const u32x4 u = *reinterpret_cast<const u32x4*>(wr + k);
      float wv[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) { wv[2 * i] = bf16lo(u[i]); wv[2 * i + 1] = bf16hi(u[i]); }
#pragma unroll
      for (int b = 0; b < GEMV_MAXB; ++b) {
        if (b < B) {
          const f32x4 a0 = *reinterpret_cast<const f32x4*>(xs + b * K + k);
          const f32x4 a1 = *reinterpret_cast<const f32x4*>(xs + b * K + k + 4);
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[b] += a0[i] * wv[i] + a1[i] * wv[4 + i];
        }
      }
    }
#pragma unroll
    for (int b = 0; b < GEMV_MAXB; ++b) {
      if (b < B) {
        float v = wave_sum(acc[b]);
        if (lane == 0) {
          if (bias) v += bf16_to_f32(bias[n]);
          if (silu_out) v = silu_f(v);
          float* yp = y + b * ldy + n;
          *yp = accumulate ? (*yp + v) : v;
        }
      }
    }
  }
}

// Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0): [cos | sin]
__global__ void timestep_embedding_kernel(const float* __restrict__ t, float* __restrict__ out, int B, int dim) {
  const int half = dim / 2;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * half) return;
  const int b = i / half, j = i - b * half;
  const float f = expf(-logf(10000.0f) * (float)j / (float)half);
  const float a = t[b] * f;
  out[b * dim + j] = cosf(a);
  out[b * dim + half + j] = sinf(a);
}

// FluxPosEmbed: fp64 angles, interleaved repeat.
__global__ void rope_table_kernel(const float* __restrict__ ids, float* __restrict__ cosv, float* __restrict__ sinv,
                                  int S, int d0, int d1, int d2, float theta) {
  const int D = d0 + d1 + d2;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S * (D / 2)) return;
  const int s = i / (D / 2);
  int j = i - s * (D / 2);        // frequency index over concatenated axes
  int axis = 0, da = d0, off = 0;
  if (j >= d0 / 2) { j -= d0 / 2; axis = 1; da = d1; off = d0; }
  if (axis == 1 && j >= d1 / 2) { j -= d1 / 2; axis = 2; da = d2; off = d0 + d1; }
  const double omega = 1.0 / pow((double)theta, (double)(2 * j) / (double)da);
  const double ang = (double)ids[s * 3 + axis] * omega;
  const float c = (float)cos(ang), sn = (float)sin(ang);
  float* cp = cosv + (int64_t)s * D + off + 2 * j;
  float* sp = sinv + (int64_t)s * D + off + 2 * j;
  cp[0] = c; cp[1] = c; sp[0] = sn; sp[1] = sn;
}

// x = bf16(x + ds·v) as the scheduler's reference computes it (oracle/flux_oracle.py euler_step; torch: x.float() + ds * v.float()):
// the product is rounded to fp32, then the sum, then the result to bf16. Contraction is off in both kernels: a fused multiply-add
// skips the product's rounding, which moves about one element in two million across a bf16 rounding boundary.
__global__ void euler_step_kernel(bf16_t* __restrict__ x, const bf16_t* __restrict__ v, float ds, int64_t n8) {
#pragma clang fp contract(off)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    u32x4 a = reinterpret_cast<u32x4*>(x)[i];
    const u32x4 b = reinterpret_cast<const u32x4*>(v)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      a[j] = pack_bf16x2(bf16lo(a[j]) + ds * bf16lo(b[j]), bf16hi(a[j]) + ds * bf16hi(b[j]));
    reinterpret_cast<u32x4*>(x)[i] = a;
  }
}
__global__ void euler_step_tail_kernel(bf16_t* x, const bf16_t* v, float ds, int64_t start, int64_t n) {
#pragma clang fp contract(off)
  const int64_t i = start + blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = f32_to_bf16(bf16_to_f32(x[i]) + ds * bf16_to_f32(v[i]));
}

// The fp32 master step, per element and all in fp32 (u, t bf16 widened; the mixed velocity is never rounded to bf16):
//   v = CFG ? u + s·(t − u) : u;   r = x + ds·v;   x = REPAINT ? (1 − m)·keep + m·r : r,   keep = (1 − sn)·src + sn·noise
// and xb, when given, receives bf16(x): the copy the next step's x_embedder reads. The three entries run instantiations of this
// one text; the tests hold them to bit equality where they must agree: t == u (the mix is u + s·0 = u exactly) and m = 1.
//
// keep and the blend are computed with contraction off, every product and sum rounded once: keep is then what torch's
// (1 − σ)·src + σ·noise gives bit for bit (scheduler.scale_noise), and with m = 1 the blend is 0·keep + r = r, with m = 0 it is
// keep + 0·r = keep, with σ = 0 keep is src + 0·noise = src, for finite inputs. The pragma stays inside repaint_blend: v and r are
// left to the compiler's default contraction.
__device__ __forceinline__ float repaint_blend(float r, float src, float noise, float m, float sn) {
#pragma clang fp contract(off)
  const float keep = (1.0f - sn) * src + sn * noise;
  return (1.0f - m) * keep + m * r;
}

// MULTI (the second-order multistep form, scheduler.FlowMatchMultistepScheduler): h holds the velocity of the step before, and
//   v2 = w != 0 ? v + w·(v − h) : v;   r = x + ds·v2;   h = v
// w is a kernel scalar, so the branch is uniform: with w = 0 (the first step of a run) h is written and never read — it may be
// uninitialised memory — and r is the text of the form without MULTI, the same bits.
// PROJ (projected guidance, rt_projected_step_f32): u carries the guidance difference d (fp32, from rt_guidance_reduce_f32), t the
// positive prediction p, s is s − 1, and k (the norm clamp) and e = (η − 1)·α are the sample's two scalars:
//   v = p + (s − 1)·(k·d + e·p)
// With d = 0 (u == p) k = 1 and e = 0, so v = p + (s − 1)·0 = p: the plain step on p, the same bits.
// STOCH (stochastic sampling, rt_stochastic_step_f32 / rt_projected_stochastic_step_f32): the predicted clean image re-noised to the
// next sigma with a fresh standard normal z (philox.h), in the Euler rule's place:
//   x0 = x − σ·v;   ê = x0 + v (only where η < 1);   n = η < 1 ? c·ê + η·z : z,  c = sqrt(1 − η²);   r = (1 − σn)·x0 + σn·n
// σn = 0 (the last step) gives r = x0 and z is never drawn: the branch is uniform, sn is a kernel scalar. Contraction off, every
// product and sum rounded once: the 16-byte and the one-element path cannot differ by what the compiler fuses in either.
struct stoch_args {
  float sigma = 0.0f, eta = 1.0f, c = 0.0f;
  uint32_t step = 0;
  int64_t seed = 0, sub = 0;
};
__device__ __forceinline__ float stochastic_rule(float x, float v, float z, float sigma, float sn, float eta, float c) {
#pragma clang fp contract(off)
  const float x0 = x - sigma * v;
  if (sn == 0.0f) return x0;
  float n = z;
  if (eta < 1.0f) n = c * (x0 + v) + eta * z;
  return (1.0f - sn) * x0 + sn * n;
}

template <bool CFG, bool REPAINT, bool MULTI, bool PROJ = false, bool STOCH = false>
__device__ __forceinline__ float master_step_element(float x, float u, float t, float src, float noise, float m, float s, float ds,
                                                     float sn, float w, float& h, float k = 1.0f, float e = 0.0f, float z = 0.0f,
                                                     const stoch_args& st = stoch_args()) {
  static_assert(!(STOCH && MULTI), "the history of a re-noised state is not a velocity of the same trajectory");
  const float v = PROJ ? t + s * (k * u + e * t) : CFG ? u + s * (t - u) : u;
  float v2 = v;
  if (MULTI) {
    if (w != 0.0f) v2 = v + w * (v - h);
    h = v;
  }
  const float r = STOCH ? stochastic_rule(x, v, z, st.sigma, sn, st.eta, st.c) : x + ds * v2;
  return REPAINT ? repaint_blend(r, src, noise, m, sn) : r;
}

// n4 groups of four elements with 16-byte loads and stores (8-byte ones for bf16), then the elements from 4·n4 on one at a time:
// the up to three left over, or all of them — the host sets n4 = 0 where a pointer is not aligned or a group could straddle the
// mask's period (n_mask < n and no multiple of 4). m = mask[i % n_mask]; t is read only under CFG, src / noise / mask only under
// REPAINT, hist only under MULTI (read where w != 0, always written), in the groups and by the tail rules of x.
// The one text of both kernels below. Under PROJ the pointers are those of one sample (n = n_s), d is its guidance difference (u is
// not read), mbase its first element's flat index for the mask's rule, and tid / nthr count over the x dimension of the grid.
// Under STOCH the pointers are one sample's too (the index inside the sample is the Philox counter), and z is drawn per group — by
// the tail per element, from the element's group — unless sn == 0.
template <bool CFG, bool REPAINT, bool MULTI, bool PROJ, bool STOCH = false>
__device__ __forceinline__ void master_step_body(float* __restrict__ x, const bf16_t* __restrict__ u, const bf16_t* __restrict__ t,
                                                 bf16_t* __restrict__ xb, const float* __restrict__ src, const float* __restrict__ noise,
                                                 const float* __restrict__ mask, float* __restrict__ hist, float s, float ds, float sn,
                                                 float w, int64_t n, int64_t n_mask, int64_t n4, int64_t tid, int64_t nthr,
                                                 const float* __restrict__ d, int64_t mbase, float k, float e,
                                                 const stoch_args& st = stoch_args()) {
  for (int64_t g = tid; g < n4; g += nthr) {
    const f32x4 xv = reinterpret_cast<const f32x4*>(x)[g];
    u32x2 uv, tv;
    f32x4 dv = xv;
    if (PROJ) {
      dv = reinterpret_cast<const f32x4*>(d)[g];
      uv = tv = reinterpret_cast<const u32x2*>(t)[g];
    } else {
      uv = reinterpret_cast<const u32x2*>(u)[g];
      tv = uv;
      if (CFG) tv = reinterpret_cast<const u32x2*>(t)[g];
    }
    f32x4 sv = xv, nv = xv, mv = xv, hv = xv;      // like tv: placeholders that the helper ignores without REPAINT / MULTI
    if (REPAINT) {
      sv = reinterpret_cast<const f32x4*>(src)[g];
      nv = reinterpret_cast<const f32x4*>(noise)[g];
      mv = *reinterpret_cast<const f32x4*>(mask + (PROJ || STOCH ? (mbase + g * 4) % n_mask : (g * 4) % n_mask));
    }
    if (MULTI && w != 0.0f) hv = reinterpret_cast<const f32x4*>(hist)[g];
    float zv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (STOCH && sn != 0.0f) philox_normal4(philox_group(st.seed, st.sub, st.step, (uint64_t)g), zv);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = PROJ ? dv[j] : (j & 1) ? bf16hi(uv[j >> 1]) : bf16lo(uv[j >> 1]);
      const float b = (j & 1) ? bf16hi(tv[j >> 1]) : bf16lo(tv[j >> 1]);
      float h = hv[j];
      o[j] = master_step_element<CFG, REPAINT, MULTI, PROJ, STOCH>(xv[j], a, b, sv[j], nv[j], mv[j], s, ds, sn, w, h, k, e, zv[j], st);
      hv[j] = h;
    }
    reinterpret_cast<f32x4*>(x)[g] = o;
    if (xb) reinterpret_cast<u32x2*>(xb)[g] = u32x2{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
    if (MULTI) reinterpret_cast<f32x4*>(hist)[g] = hv;
  }
  for (int64_t i = n4 * 4 + tid; i < n; i += nthr) {
    float a, b;
    if (PROJ) { a = d[i]; b = bf16_to_f32(t[i]); }
    else { a = bf16_to_f32(u[i]); b = CFG ? bf16_to_f32(t[i]) : a; }
    float sv = 0.0f, nv = 0.0f, mv = 0.0f, h = 0.0f;
    if (REPAINT) { sv = src[i]; nv = noise[i]; mv = mask[PROJ || STOCH ? (mbase + i) % n_mask : i % n_mask]; }
    if (MULTI && w != 0.0f) h = hist[i];
    float z = 0.0f;
    if (STOCH && sn != 0.0f) z = philox_normal_lane(philox_group(st.seed, st.sub, st.step, (uint64_t)(i >> 2)), (int)(i & 3));
    const float o = master_step_element<CFG, REPAINT, MULTI, PROJ, STOCH>(x[i], a, b, sv, nv, mv, s, ds, sn, w, h, k, e, z, st);
    x[i] = o;
    if (xb) xb[i] = f32_to_bf16(o);
    if (MULTI) hist[i] = h;
  }
}

template <bool CFG, bool REPAINT, bool MULTI>
__global__ void master_step_f32_kernel(float* __restrict__ x, const bf16_t* __restrict__ u, const bf16_t* __restrict__ t,
                                       bf16_t* __restrict__ xb, const float* __restrict__ src, const float* __restrict__ noise,
                                       const float* __restrict__ mask, float* __restrict__ hist, float s, float ds, float sn, float w,
                                       int64_t n, int64_t n_mask, int64_t n4) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  master_step_body<CFG, REPAINT, MULTI, false>(x, u, t, xb, src, noise, mask, hist, s, ds, sn, w, n, n_mask, n4, tid, nthr, nullptr, 0,
                                               1.0f, 0.0f);
}

// The stochastic forms: grid (x, B), the pointers of sample blockIdx.y, whose (seed, subsequence) is row blockIdx.y of rng — read
// only where a z is drawn (sn != 0), so the last step never touches it.
__device__ __forceinline__ stoch_args stoch_args_of(const int64_t* __restrict__ rng, float sigma, float sn, float eta, float c, uint32_t step) {
  stoch_args st;
  st.sigma = sigma; st.eta = eta; st.c = c; st.step = step;
  if (sn != 0.0f) { st.seed = rng[2 * (int64_t)blockIdx.y]; st.sub = rng[2 * (int64_t)blockIdx.y + 1]; }
  return st;
}

template <bool CFG, bool REPAINT>
__global__ void stochastic_step_f32_kernel(float* __restrict__ x, const bf16_t* __restrict__ u, const bf16_t* __restrict__ t,
                                           bf16_t* __restrict__ xb, const float* __restrict__ src, const float* __restrict__ noise,
                                           const float* __restrict__ mask, const int64_t* __restrict__ rng, float s, float sigma, float sn,
                                           float eta, float c, uint32_t step, int64_t n_s, int64_t n_mask, int64_t n4) {
  const stoch_args st = stoch_args_of(rng, sigma, sn, eta, c, step);
  const int64_t base = (int64_t)blockIdx.y * n_s;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  master_step_body<CFG, REPAINT, false, false, true>(x + base, u + base, CFG ? t + base : nullptr, xb ? xb + base : nullptr,
                                                     REPAINT ? src + base : nullptr, REPAINT ? noise + base : nullptr, mask, nullptr, s, 0.0f,
                                                     sn, 0.0f, n_s, n_mask, n4, tid, nthr, nullptr, base, 1.0f, 0.0f, st);
}

// out[b][i] = the z the stochastic step draws for element i of sample b at ``step``: the same two paths, the same bits
__global__ void normal_fill_f32_kernel(float* __restrict__ out, const int64_t* __restrict__ rng, uint32_t step, int64_t n_s, int64_t n4) {
  const int64_t seed = rng[2 * (int64_t)blockIdx.y], sub = rng[2 * (int64_t)blockIdx.y + 1];
  out += (int64_t)blockIdx.y * n_s;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  for (int64_t g = tid; g < n4; g += nthr) {
    float z[4];
    philox_normal4(philox_group(seed, sub, step, (uint64_t)g), z);
    reinterpret_cast<f32x4*>(out)[g] = f32x4{z[0], z[1], z[2], z[3]};
  }
  for (int64_t i = n4 * 4 + tid; i < n_s; i += nthr)
    out[i] = philox_normal_lane(philox_group(seed, sub, step, (uint64_t)(i >> 2)), (int)(i & 3));
}

// ---- projected guidance: per-sample sums, then the master step with the projected velocity (reptext_hip.h) --------------------------
// One term of the three sums and the difference itself. Contraction off: every product and sum is rounded once, so the 16-byte and
// the one-element path of the kernel below cannot differ by what the compiler fuses in either.
__device__ __forceinline__ float guidance_term(float p, float u, float r, float beta, float& a, float& b, float& c) {
#pragma clang fp contract(off)
  float d = p - u;
  if (beta != 0.0f) d = d + beta * r;
  a += d * d;
  b += d * p;
  c += p * p;
  return d;
}

// grid (chunks, B), 256 threads: thread th takes the groups of four th, th + 256, th + 512, th + 768 of its chunk of RT_GUIDE_CHUNK
// elements, in that order and the four elements of a group in theirs, whether it loads them as a group (VEC) or one by one.
template <bool VEC>
__global__ __launch_bounds__(256) void guidance_reduce_kernel(const bf16_t* __restrict__ u, const bf16_t* __restrict__ t,
                                                              float* __restrict__ diff, float beta, float* __restrict__ partials,
                                                              int64_t n_s) {
  static_assert(RT_GUIDE_CHUNK == 4 * 4 * 256, "four groups of four per thread");
  const int64_t base = (int64_t)blockIdx.y * n_s;
  u += base; t += base; diff += base;
  float a = 0.0f, b = 0.0f, c = 0.0f;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int64_t o = (int64_t)blockIdx.x * RT_GUIDE_CHUNK + (it * 256 + (int)threadIdx.x) * 4;
    if (VEC) {
      if (o < n_s) {              // n_s % 4 == 0: a group is inside the sample or outside it
        const u32x2 uv = *reinterpret_cast<const u32x2*>(u + o), tv = *reinterpret_cast<const u32x2*>(t + o);
        f32x4 rv = {0.0f, 0.0f, 0.0f, 0.0f};
        if (beta != 0.0f) rv = *reinterpret_cast<const f32x4*>(diff + o);
        f32x4 dv;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          dv[j] = guidance_term((j & 1) ? bf16hi(tv[j >> 1]) : bf16lo(tv[j >> 1]), (j & 1) ? bf16hi(uv[j >> 1]) : bf16lo(uv[j >> 1]),
                                rv[j], beta, a, b, c);
        *reinterpret_cast<f32x4*>(diff + o) = dv;
      }
    } else {
      for (int j = 0; j < 4; ++j)
        if (o + j < n_s) {
          const float r = beta != 0.0f ? diff[o + j] : 0.0f;
          diff[o + j] = guidance_term(bf16_to_f32(t[o + j]), bf16_to_f32(u[o + j]), r, beta, a, b, c);
        }
    }
  }
  a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
  __shared__ float red[4][3];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[wave][0] = a; red[wave][1] = b; red[wave][2] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* out = partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
#pragma unroll
    for (int q = 0; q < 3; ++q) out[q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
  }
}

// grid (x, B). Prologue, the same in every workgroup of a sample: its partials added in index order in double, k and e formed in
// double and rounded to float once. Then the one step body on the sample's pointers.
template <bool REPAINT, bool MULTI>
__global__ void projected_step_f32_kernel(float* __restrict__ x, const bf16_t* __restrict__ t, bf16_t* __restrict__ xb,
                                          const float* __restrict__ diff, const float* __restrict__ partials, int nparts, float s1,
                                          float eta, float tau, const float* __restrict__ src, const float* __restrict__ noise,
                                          const float* __restrict__ mask, float* __restrict__ hist, float ds, float sn, float w,
                                          int64_t n_s, int64_t n_mask, int64_t n4) {
  const float* part = partials + (int64_t)blockIdx.y * nparts * 3;
  double a = 0.0, b = 0.0, c = 0.0;
  for (int j = 0; j < nparts; ++j) { a += (double)part[3 * j]; b += (double)part[3 * j + 1]; c += (double)part[3 * j + 2]; }
  const double kd = (tau > 0.0f && a > (double)tau * (double)tau) ? (double)tau / sqrt(a) : 1.0;
  const double alpha = c > 0.0 ? kd * b / c : 0.0;
  const float k = (float)kd, e = (float)(((double)eta - 1.0) * alpha);
  const int64_t base = (int64_t)blockIdx.y * n_s;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  master_step_body<false, REPAINT, MULTI, true>(x + base, nullptr, t + base, xb ? xb + base : nullptr, REPAINT ? src + base : nullptr,
                                                REPAINT ? noise + base : nullptr, mask, MULTI ? hist + base : nullptr, s1, ds, sn, w,
                                                n_s, n_mask, n4, tid, nthr, diff + base, base, k, e);
}

// The projected step's stochastic form: the same prologue, then the STOCH body (no history).
template <bool REPAINT>
__global__ void projected_stochastic_step_f32_kernel(float* __restrict__ x, const bf16_t* __restrict__ t, bf16_t* __restrict__ xb,
                                                     const float* __restrict__ diff, const float* __restrict__ partials, int nparts, float s1,
                                                     float eta_g, float tau, const float* __restrict__ src, const float* __restrict__ noise,
                                                     const float* __restrict__ mask, const int64_t* __restrict__ rng, float sigma, float sn,
                                                     float eta, float c, uint32_t step, int64_t n_s, int64_t n_mask, int64_t n4) {
  const float* part = partials + (int64_t)blockIdx.y * nparts * 3;
  double a = 0.0, b = 0.0, cc = 0.0;
  for (int j = 0; j < nparts; ++j) { a += (double)part[3 * j]; b += (double)part[3 * j + 1]; cc += (double)part[3 * j + 2]; }
  const double kd = (tau > 0.0f && a > (double)tau * (double)tau) ? (double)tau / sqrt(a) : 1.0;
  const double alpha = cc > 0.0 ? kd * b / cc : 0.0;
  const float k = (float)kd, e = (float)(((double)eta_g - 1.0) * alpha);
  const stoch_args st = stoch_args_of(rng, sigma, sn, eta, c, step);
  const int64_t base = (int64_t)blockIdx.y * n_s;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  master_step_body<false, REPAINT, false, true, true>(x + base, nullptr, t + base, xb ? xb + base : nullptr, REPAINT ? src + base : nullptr,
                                                      REPAINT ? noise + base : nullptr, mask, nullptr, s1, 0.0f, sn, 0.0f, n_s, n_mask, n4, tid,
                                                      nthr, diff + base, base, k, e, st);
}

__global__ void cfg_mix_kernel(const bf16_t* __restrict__ u, const bf16_t* __restrict__ t, bf16_t* __restrict__ o,
                               float s, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float a = bf16_to_f32(u[i]), b = bf16_to_f32(t[i]);
    o[i] = f32_to_bf16(a + s * (b - a));
  }
}

// packed[b][(i*W+j)][c*4+dy*2+dx] = x[b][c][2i+dy][2j+dx]
__global__ void pack_latents_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ p, int B, int C, int H2, int W2) {
  const int64_t n = (int64_t)B * C * H2 * W2;
  const int h = H2 / 2, w = W2 / 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = i;
    const int ch = (int)(t % (C * 4)); t /= (C * 4);
    const int j = (int)(t % w); t /= w;
    const int ii = (int)(t % h);
    const int b = (int)(t / h);
    const int c = ch >> 2, dy = (ch >> 1) & 1, dx = ch & 1;
    p[i] = x[(((int64_t)b * C + c) * H2 + (2 * ii + dy)) * W2 + 2 * j + dx];
  }
}
// inverse, with z/scaling + shift, output NHWC bf16 [B][H2][W2][C]
__global__ void unpack_latents_kernel(const bf16_t* __restrict__ p, bf16_t* __restrict__ y, int B, int C, int H2, int W2,
                                      float inv_scale, float shift) {
  const int64_t n = (int64_t)B * C * H2 * W2;
  const int h = H2 / 2, w = W2 / 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = i;
    const int c = (int)(t % C); t /= C;
    const int xx = (int)(t % W2); t /= W2;
    const int yy = (int)(t % H2);
    const int b = (int)(t / H2);
    const int tok = (yy >> 1) * w + (xx >> 1);
    const int ch = c * 4 + (yy & 1) * 2 + (xx & 1);
    const float v = bf16_to_f32(p[((int64_t)b * h * w + tok) * (C * 4) + ch]);
    y[i] = f32_to_bf16(v * inv_scale + shift);
  }
}

__global__ void cast_f32_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = f32_to_bf16(x[i]);
}
__global__ void cast_bf16_f32_kernel(const bf16_t* __restrict__ x, float* __restrict__ y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = bf16_to_f32(x[i]);
}

// fp32 destination variant (fp32 residual stream): y[b][r][:] (+)= alpha * rowscale[r] * x[b][r][:]
__global__ void masked_accumulate_f32_kernel(const bf16_t* __restrict__ x, float* __restrict__ y,
                                             const float* __restrict__ rowscale, float alpha, int batch, int rows, int D8,
                                             int accumulate) {
  const int64_t n = (int64_t)batch * rows * D8;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)((i / D8) % rows);
    const float m = alpha * (rowscale ? rowscale[r] : 1.0f);
    const u32x4 a = reinterpret_cast<const u32x4*>(x)[i];
    f32x4 lo = f32x4{bf16lo(a[0]), bf16hi(a[0]), bf16lo(a[1]), bf16hi(a[1])} * m;
    f32x4 hi = f32x4{bf16lo(a[2]), bf16hi(a[2]), bf16lo(a[3]), bf16hi(a[3])} * m;
    f32x4* yp = reinterpret_cast<f32x4*>(y) + 2 * i;
    if (accumulate) { lo += yp[0]; hi += yp[1]; }
    yp[0] = lo; yp[1] = hi;
  }
}

// y[b][r][:] (+)= alpha * rowscale[r] * x[b][r][:], 8 elements per lane
__global__ void masked_accumulate_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                         const float* __restrict__ rowscale, float alpha, int batch, int rows, int D8,
                                         int accumulate) {
  const int64_t n = (int64_t)batch * rows * D8;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)((i / D8) % rows);
    const float m = alpha * (rowscale ? rowscale[r] : 1.0f);
    const u32x4 a = reinterpret_cast<const u32x4*>(x)[i];
    u32x4 o;
    if (accumulate) {
      const u32x4 c = reinterpret_cast<const u32x4*>(y)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        o[j] = pack_bf16x2(bf16lo(c[j]) + m * bf16lo(a[j]), bf16hi(c[j]) + m * bf16hi(a[j]));
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(m * bf16lo(a[j]), m * bf16hi(a[j]));
    }
    reinterpret_cast<u32x4*>(y)[i] = o;
  }
}

// hi = bf16(silu(x)), lo = bf16(silu(x) - hi): two-term bf16 split so a bf16 MFMA GEMM reproduces an fp32-activation product
__global__ void silu_split_kernel(const float* __restrict__ x, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, int64_t n,
                                  int apply_silu) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = apply_silu ? silu_f(x[i]) : x[i];
    const bf16_t h = f32_to_bf16(v);
    hi[i] = h;
    lo[i] = f32_to_bf16(v - bf16_to_f32(h));
  }
}

// y[r][:] = (y[r][:] + a[r % B][:]) + b[r % B][:], 4 floats per thread (time_text_embed for all steps: (t + g) + p)
__global__ void add_rows_f32_kernel(float* __restrict__ y, const float* __restrict__ a, const float* __restrict__ b, int rows, int B, int D4) {
  const int64_t n = (int64_t)rows * D4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / D4), c = (int)(i - (int64_t)r * D4);
    const int64_t j = (int64_t)(r % B) * D4 + c;
    f32x4 v = reinterpret_cast<const f32x4*>(y)[i] + reinterpret_cast<const f32x4*>(a)[j];
    if (b) v += reinterpret_cast<const f32x4*>(b)[j];
    reinterpret_cast<f32x4*>(y)[i] = v;
  }
}

// Compile-time choice of a row kernel's instance: f(integral_constant<int, N>) for the first N of the list with nch <= N, and for
// the last of the list when there is none (the widest instance, or 0 = the instance that strides the row).
template <int N0, int... Ns, class F>
void for_nch(int nch, F f) {
  if constexpr (sizeof...(Ns) == 0) f(std::integral_constant<int, N0>{});
  else if (nch <= N0) f(std::integral_constant<int, N0>{});
  else for_nch<Ns...>(nch, f);
}

// e4m3 output with row scales: instances {2, 6, 16}; bf16 output: instances {1, 2, 4, 6, 8, 16}.
int launch_layernorm(const LnLaunch& L, int x_f32, bool out_fp8, float* row_scale, int D, float eps, void* stream) {
  const dim3 grid((L.rows + 3) / 4), block(256);
  hipStream_t st = (hipStream_t)stream;
  const int nch = (D + 511) / 512;
  auto with_x = [&](auto f32) {
    constexpr bool F32 = decltype(f32)::value;
    if (out_fp8)
      for_nch<2, 6, 16>(nch, [&](auto n) {
        hipLaunchKernelGGL((layernorm_mod_kernel<F32, decltype(n)::value, true>), grid, block, 0, st, L, D, eps, row_scale);
      });
    else
      for_nch<1, 2, 4, 6, 8, 16>(nch, [&](auto n) {
        hipLaunchKernelGGL((layernorm_mod_kernel<F32, decltype(n)::value, false>), grid, block, 0, st, L, D, eps, row_scale);
      });
  };
  if (x_f32) with_x(std::true_type{}); else with_x(std::false_type{});
  return rt_hip_status();
}

// The refusals of one segment: its arguments, then its alignment (out_align: 16 for bf16 output, 8 for e4m3).
int check_ln_segment(const rt_ln_segment& g, int out_align) {
  if (!g.x || !g.out || g.batch < 1 || g.rows_per_batch < 1) return RT_E_BADARG;
  if ((g.shift == nullptr) != (g.scale == nullptr)) return RT_E_BADARG;
  if (!RT_ALIGNED(g.x, 16) || !RT_ALIGNED(g.out, out_align) || g.ldx % 8 || g.ldo % 8 || g.stride_xb % 8 || g.stride_ob % 8) return RT_E_ALIGN;
  if (g.scale && (!RT_ALIGNED(g.scale, 16) || !RT_ALIGNED(g.shift, 16) || g.mod_ld % 4)) return RT_E_ALIGN;
  return RT_OK;
}

// The two entries of one segment: argument refusals, then the shape of D, then alignment.
int layernorm_one_segment(const rt_ln_segment& g, int x_f32, bool out_fp8, float* row_scale, int D, float eps, void* stream) {
  const int refusal = check_ln_segment(g, out_fp8 ? 8 : 16);
  if (refusal == RT_E_BADARG || (out_fp8 && !row_scale) || D < 8) return RT_E_BADARG;
  if (D % 8 || D > 8192) return RT_E_SHAPE;
  if (refusal) return refusal;
  LnLaunch L{};
  L.seg[0] = g;
  L.rows0 = L.rows = g.batch * g.rows_per_batch;
  return launch_layernorm(L, x_f32, out_fp8, row_scale, D, eps, stream);
}

// y = bf16(gelu(x)), the exact (erf) form 0.5 x (1 + erf(x / sqrt 2)): the InstantX image projection's activation (the GEMM epilogue
// has the tanh form only). x fp32 as the GEMM wrote it, so the hidden is rounded once.
__global__ void gelu_erf_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = x[i];
    y[i] = f32_to_bf16(0.5f * v * (1.0f + erff(v * 0.70710678118654752f)));
  }
}

// y[b][r][:] = bf16(y[b][r][:] + x[b][r][:]) on bf16 views with their own row and batch strides, 8 elements per lane
__global__ void add_bf16_2d_kernel(const bf16_t* __restrict__ x, int64_t ldx, int64_t stride_xb, bf16_t* __restrict__ y, int64_t ldy,
                                   int64_t stride_yb, int batch, int rows, int D8) {
  const int64_t n = (int64_t)batch * rows * D8;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % D8);
    const int64_t br = i / D8;
    const int r = (int)(br % rows), b = (int)(br / rows);
    const u32x4 a = *reinterpret_cast<const u32x4*>(x + b * stride_xb + r * ldx + 8 * c);
    u32x4* yp = reinterpret_cast<u32x4*>(y + b * stride_yb + r * ldy + 8 * c);
    const u32x4 o = *yp;
    u32x4 w;
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = pack_bf16x2(bf16lo(o[j]) + bf16lo(a[j]), bf16hi(o[j]) + bf16hi(a[j]));
    *yp = w;
  }
}

}  // namespace

extern "C" {

int rt_layernorm_modulate(const void* x, int64_t ldx, int64_t stride_xb, int32_t x_f32, void* out, int64_t ldo,
                          int64_t stride_ob, const float* shift, const float* scale, int64_t mod_ld, int32_t batch,
                          int32_t rows_per_batch, int32_t D, float eps, void* stream) {
  return layernorm_one_segment(rt_ln_segment{x, out, shift, scale, ldx, stride_xb, ldo, stride_ob, mod_ld, batch, rows_per_batch}, x_f32,
                               false, nullptr, D, eps, stream);
}

int rt_layernorm_modulate_pair(const rt_ln_segment* segs, int32_t x_f32, int32_t D, float eps, void* stream) {
  if (!segs || D < 8) return RT_E_BADARG;
  if (D % 8 || D > 8192) return RT_E_SHAPE;
  LnLaunch L{};
  for (int i = 0; i < 2; ++i) {
    if (const int refusal = check_ln_segment(segs[i], 16)) return refusal;
    L.seg[i] = segs[i];
  }
  L.rows0 = segs[0].batch * segs[0].rows_per_batch;
  L.rows = L.rows0 + segs[1].batch * segs[1].rows_per_batch;
  return launch_layernorm(L, x_f32, false, nullptr, D, eps, stream);
}

int rt_layernorm_modulate_fp8(const void* x, int64_t ldx, int64_t stride_xb, int32_t x_f32, void* out, int64_t ldo,
                              int64_t stride_ob, float* row_scale, const float* shift, const float* scale, int64_t mod_ld,
                              int32_t batch, int32_t rows_per_batch, int32_t D, float eps, void* stream) {
  return layernorm_one_segment(rt_ln_segment{x, out, shift, scale, ldx, stride_xb, ldo, stride_ob, mod_ld, batch, rows_per_batch}, x_f32,
                               true, row_scale, D, eps, stream);
}

int rt_quantize_rows_fp8(const void* x, int64_t ldx, int32_t x_f32, void* out, int64_t ldo, float* scale, int32_t rows,
                         int32_t D, void* stream) {
  if (!x || !out || !scale || rows < 1 || D < 8) return RT_E_BADARG;
  if (D % 8 || D > 65536) return RT_E_SHAPE;
  if (!RT_ALIGNED(x, 16) || !RT_ALIGNED(out, 8) || ldx % 8 || ldo % 8) return RT_E_ALIGN;
  const dim3 grid((rows + 3) / 4), block(256);
  hipStream_t st = (hipStream_t)stream;
  const int nch = (D + 511) / 512;
  auto launch = [&](auto f32, auto n) {
    hipLaunchKernelGGL((quantize_rows_fp8_kernel<decltype(f32)::value, decltype(n)::value>), grid, block, 0, st, x, ldx, (uint8_t*)out, ldo,
                       scale, rows, D);
  };
  if (x_f32) launch(std::true_type{}, std::integral_constant<int, 0>{});
  else for_nch<6, 12, 24, 30, 0>(nch, [&](auto n) { launch(std::false_type{}, n); });   // rows above 64·8·30 elements: two passes
  return rt_hip_status();
}

int rt_quantize_mx_fp8(const void* x, int64_t ldx, int32_t x_f32, void* out, int64_t ldo, uint8_t* bscale, int64_t plane,
                       int32_t rows, int32_t D, void* stream) {
  if (!x || !out || !bscale || rows < 1 || D < 256) return RT_E_BADARG;
  if (D % 256 || plane % 2048 || plane < (((int64_t)rows + 63) / 64) * 2048) return RT_E_SHAPE;
  if (!RT_ALIGNED(x, 16) || !RT_ALIGNED(out, 8) || ldx % 8 || ldo % 8 || !RT_ALIGNED(bscale, 16)) return RT_E_ALIGN;
  const int64_t n = (int64_t)rows * (D / 8);
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (x_f32) hipLaunchKernelGGL(quantize_mx_fp8_kernel<true>, grid, block, 0, st, x, ldx, (uint8_t*)out, ldo, bscale, plane, rows, D);
  else hipLaunchKernelGGL(quantize_mx_fp8_kernel<false>, grid, block, 0, st, x, ldx, (uint8_t*)out, ldo, bscale, plane, rows, D);
  return rt_hip_status();
}

int rt_qk_rmsnorm_rope(void* buf, int64_t ld, int64_t stride_b, int64_t q_off, int64_t k_off, const void* wq_txt,
                       const void* wk_txt, const void* wq_img, const void* wk_img, const float* cosv,
                       const float* sinv, int32_t B, int32_t S, int32_t T, int32_t H, float eps, void* stream) {
  if (!buf || !wq_img || !wk_img || !cosv || !sinv || B < 1 || S < 1 || H < 1 || T < 0 || T > S) return RT_E_BADARG;
  if (T > 0 && (!wq_txt || !wk_txt)) return RT_E_BADARG;
  if (!RT_ALIGNED(buf, 16) || ld % 8 || stride_b % 8 || q_off % 8 || k_off % 8 || !RT_ALIGNED(cosv, 16) ||
      !RT_ALIGNED(sinv, 16) || !RT_ALIGNED(wq_img, 16) || !RT_ALIGNED(wk_img, 16))
    return RT_E_ALIGN;
  if (T > 0 && (!RT_ALIGNED(wq_txt, 16) || !RT_ALIGNED(wk_txt, 16))) return RT_E_ALIGN;   // loaded as 16-byte vectors like the image weights
  const int64_t ngrp = (int64_t)B * S * ((H + QK_HC - 1) / QK_HC);
  const int64_t blocks = (ngrp + 15) / 16;
  if (blocks > 0x7fffffff) return RT_E_SHAPE;
  hipLaunchKernelGGL(qk_rmsnorm_rope_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     (bf16_t*)buf, ld, stride_b, q_off, k_off, (const bf16_t*)wq_txt, (const bf16_t*)wk_txt,
                     (const bf16_t*)wq_img, (const bf16_t*)wk_img, cosv, sinv, B, S, T, H, eps);
  return rt_hip_status();
}

int rt_gemv_bf16w(const float* x, int64_t ldx, const void* W, int64_t ldw, const void* bias, float* y, int64_t ldy,
                  int32_t B, int32_t N, int32_t K, int32_t silu_in, int32_t silu_out, int32_t accumulate,
                  void* stream) {
  if (!x || !W || !y || B < 1 || N < 1 || K < 1) return RT_E_BADARG;
  if (B > GEMV_MAXB || K % 8 || (int64_t)B * K * 4 > 64 * 1024) return RT_E_SHAPE;
  if (!RT_ALIGNED(W, 16) || ldw % 8) return RT_E_ALIGN;
  const int rows_per_block = 16;
  hipLaunchKernelGGL(gemv_bf16w_kernel, dim3((N + rows_per_block - 1) / rows_per_block), dim3(256),
                     (size_t)B * K * 4, (hipStream_t)stream, x, ldx, (const bf16_t*)W, ldw, (const bf16_t*)bias, y,
                     ldy, B, N, K, silu_in, silu_out, accumulate);
  return rt_hip_status();
}

int rt_add_rows_f32(float* y, const float* a, const float* b, int32_t rows, int32_t B, int32_t D, void* stream) {
  if (!y || !a || rows < 1 || B < 1 || D < 4) return RT_E_BADARG;
  if (D % 4) return RT_E_SHAPE;
  if (!RT_ALIGNED(y, 16) || !RT_ALIGNED(a, 16) || (b && !RT_ALIGNED(b, 16))) return RT_E_ALIGN;
  return launch_1d(add_rows_f32_kernel, (int64_t)rows * (D / 4), stream, y, a, b, rows, B, D / 4);
}

int rt_timestep_embedding(const float* t, float* out, int32_t B, int32_t dim, void* stream) {
  if (!t || !out || B < 1 || dim < 2 || dim % 2) return RT_E_BADARG;
  const int n = B * dim / 2;
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, t, out, B, dim);
  return rt_hip_status();
}

int rt_rope_table(const float* ids, float* cos_out, float* sin_out, int32_t S, const int32_t* axes_dim, float theta,
                  void* stream) {
  if (!ids || !cos_out || !sin_out || !axes_dim || S < 1) return RT_E_BADARG;
  const int d0 = axes_dim[0], d1 = axes_dim[1], d2 = axes_dim[2];
  if (d0 < 2 || d1 < 2 || d2 < 2 || d0 % 2 || d1 % 2 || d2 % 2) return RT_E_SHAPE;
  const int n = S * ((d0 + d1 + d2) / 2);
  hipLaunchKernelGGL(rope_table_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, ids, cos_out, sin_out,
                     S, d0, d1, d2, theta);
  return rt_hip_status();
}

// The one launcher of master_step_f32_kernel: v_text selects CFG, mask selects REPAINT (src and noise come with it), hist selects
// MULTI. The 16-byte path needs every pointer that is present aligned for its access and, with a mask, no group of four across the
// mask's period.
static int launch_master_step_f32(float* x, const void* v, const void* v_text, void* x_bf16, const float* src, const float* noise,
                                  const float* mask, float* hist, float s, float ds, float sn, float w, int64_t n, int64_t n_mask,
                                  void* stream) {
  const bool vec = RT_ALIGNED(x, 16) && RT_ALIGNED(v, 8) && (!v_text || RT_ALIGNED(v_text, 8)) && (!x_bf16 || RT_ALIGNED(x_bf16, 8)) &&
                   (!mask || ((n_mask % 4 == 0 || n_mask == n) && RT_ALIGNED(src, 16) && RT_ALIGNED(noise, 16) && RT_ALIGNED(mask, 16))) &&
                   (!hist || RT_ALIGNED(hist, 16));
  const int64_t n4 = vec ? n / 4 : 0;
  const auto plain = mask ? (v_text ? master_step_f32_kernel<true, true, false> : master_step_f32_kernel<false, true, false>)
                          : (v_text ? master_step_f32_kernel<true, false, false> : master_step_f32_kernel<false, false, false>);
  const auto multi = mask ? (v_text ? master_step_f32_kernel<true, true, true> : master_step_f32_kernel<false, true, true>)
                          : (v_text ? master_step_f32_kernel<true, false, true> : master_step_f32_kernel<false, false, true>);
  const auto kernel = hist ? multi : plain;
  hipLaunchKernelGGL(kernel, dim3(grid_for(n4 > 0 ? n4 : n, 256)), dim3(256), 0, (hipStream_t)stream, x, (const bf16_t*)v,
                     (const bf16_t*)v_text, (bf16_t*)x_bf16, src, noise, mask, hist, s, ds, sn, w, n, n_mask, n4);
  return rt_hip_status();
}

int rt_euler_step(void* x, const void* v, float dsigma, int64_t n, void* stream) {
  if (!x || !v || n < 1) return RT_E_BADARG;
  if (!RT_ALIGNED(x, 16) || !RT_ALIGNED(v, 16)) return RT_E_ALIGN;
  const int64_t n8 = n / 8;
  if (n8 > 0)
    hipLaunchKernelGGL(euler_step_kernel, dim3(grid_for(n8, 256)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)x,
                       (const bf16_t*)v, dsigma, n8);
  if (n8 * 8 < n)
    hipLaunchKernelGGL(euler_step_tail_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (bf16_t*)x, (const bf16_t*)v,
                       dsigma, n8 * 8, n);
  return rt_hip_status();
}

int rt_euler_step_f32(float* x, const void* v, void* x_bf16, float dsigma, int64_t n, void* stream) {
  if (!x || !v || n < 1) return RT_E_BADARG;
  return launch_master_step_f32(x, v, nullptr, x_bf16, nullptr, nullptr, nullptr, nullptr, 0.0f, dsigma, 0.0f, 0.0f, n, n, stream);
}

int rt_cfg_euler_step_f32(float* x, const void* v_uncond, const void* v_text, void* x_bf16, float s, float dsigma, int64_t n,
                          void* stream) {
  if (!x || !v_uncond || !v_text || n < 1) return RT_E_BADARG;
  return launch_master_step_f32(x, v_uncond, v_text, x_bf16, nullptr, nullptr, nullptr, nullptr, s, dsigma, 0.0f, 0.0f, n, n, stream);
}

int rt_repaint_euler_step_f32(float* x, const void* v, const void* v_text, void* x_bf16, const float* src, const float* noise,
                              const float* mask, float s, float dsigma, float sigma_next, int64_t n, int64_t n_mask, void* stream) {
  if (!x || !v || !src || !noise || !mask || n < 1 || n_mask < 1) return RT_E_BADARG;
  if (n % n_mask) return RT_E_SHAPE;
  return launch_master_step_f32(x, v, v_text, x_bf16, src, noise, mask, nullptr, s, dsigma, sigma_next, 0.0f, n, n_mask, stream);
}

int rt_multistep_step_f32(float* x, const void* v, const void* v_text, void* x_bf16, float* hist, float w, const float* src,
                          const float* noise, const float* mask, float s, float dsigma, float sigma_next, int64_t n, int64_t n_mask,
                          void* stream) {
  if (!x || !v || !hist || n < 1 || n_mask < 1 || (mask && (!src || !noise))) return RT_E_BADARG;
  if (n % n_mask) return RT_E_SHAPE;
  return launch_master_step_f32(x, v, v_text, x_bf16, src, noise, mask, hist, s, dsigma, sigma_next, w, n, n_mask, stream);
}

int64_t rt_guidance_ws_bytes(int32_t B, int64_t n_s) {
  if (B < 1 || n_s < 1) return 0;
  return (int64_t)B * ((n_s + RT_GUIDE_CHUNK - 1) / RT_GUIDE_CHUNK) * 3 * (int64_t)sizeof(float);
}

int rt_guidance_reduce_f32(const void* v_uncond, const void* v_text, float* diff, float beta, float* partials, int32_t B, int64_t n_s,
                           void* stream) {
  if (!v_uncond || !v_text || !diff || !partials || B < 1 || n_s < 1) return RT_E_BADARG;
  const int64_t chunks = (n_s + RT_GUIDE_CHUNK - 1) / RT_GUIDE_CHUNK;
  if (B > 65535 || chunks > 0x7fffffff) return RT_E_SHAPE;
  const bool vec = n_s % 4 == 0 && RT_ALIGNED(v_uncond, 8) && RT_ALIGNED(v_text, 8) && RT_ALIGNED(diff, 16);
  hipLaunchKernelGGL(vec ? guidance_reduce_kernel<true> : guidance_reduce_kernel<false>, dim3((unsigned)chunks, (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, (const bf16_t*)v_uncond, (const bf16_t*)v_text, diff, beta, partials, n_s);
  return rt_hip_status();
}

int rt_projected_step_f32(float* x, const void* v_uncond, const void* v_text, void* x_bf16, const float* diff, const float* partials,
                          float s_minus_1, float eta, float tau, float* hist, float w, const float* src, const float* noise,
                          const float* mask, float dsigma, float sigma_next, int32_t B, int64_t n_s, int64_t n_mask, void* stream) {
  if (!x || !v_uncond || !v_text || !diff || !partials || B < 1 || n_s < 1 || n_mask < 1 || (mask && (!src || !noise))) return RT_E_BADARG;
  const int64_t chunks = (n_s + RT_GUIDE_CHUNK - 1) / RT_GUIDE_CHUNK;
  if (B > 65535 || chunks > 0x7fffffff || ((int64_t)B * n_s) % n_mask) return RT_E_SHAPE;
  // every sample's pointers are aligned when the first one's are and n_s % 4 == 0; a mask's period is then a multiple of 4 too, or
  // it is the whole of [B][n_s]
  const bool vec = n_s % 4 == 0 && RT_ALIGNED(x, 16) && RT_ALIGNED(v_text, 8) && RT_ALIGNED(diff, 16) && (!x_bf16 || RT_ALIGNED(x_bf16, 8)) &&
                   (!mask || ((n_mask % 4 == 0 || n_mask == (int64_t)B * n_s) && RT_ALIGNED(src, 16) && RT_ALIGNED(noise, 16) &&
                              RT_ALIGNED(mask, 16))) &&
                   (!hist || RT_ALIGNED(hist, 16));
  const int64_t n4 = vec ? n_s / 4 : 0;
  const auto kernel = mask ? (hist ? projected_step_f32_kernel<true, true> : projected_step_f32_kernel<true, false>)
                           : (hist ? projected_step_f32_kernel<false, true> : projected_step_f32_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(grid_for(n4 > 0 ? n4 : n_s, 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, x,
                     (const bf16_t*)v_text, (bf16_t*)x_bf16, diff, partials, (int)chunks, s_minus_1, eta, tau, src, noise, mask, hist, dsigma,
                     sigma_next, w, n_s, n_mask, n4);
  return rt_hip_status();
}

// The 16-byte path of the stochastic forms: as above, and n_s % 4 == 0 — a group is one Philox call, so none may straddle two samples.
static bool stochastic_vec(const float* x, const void* v, const void* v_text, const void* x_bf16, const float* src, const float* noise,
                           const float* mask, int32_t B, int64_t n_s, int64_t n_mask) {
  return n_s % 4 == 0 && RT_ALIGNED(x, 16) && (!v || RT_ALIGNED(v, 8)) && (!v_text || RT_ALIGNED(v_text, 8)) && (!x_bf16 || RT_ALIGNED(x_bf16, 8)) &&
         (!mask || ((n_mask % 4 == 0 || n_mask == (int64_t)B * n_s) && RT_ALIGNED(src, 16) && RT_ALIGNED(noise, 16) && RT_ALIGNED(mask, 16)));
}

int rt_stochastic_step_f32(float* x, const void* v, const void* v_text, void* x_bf16, const float* src, const float* noise, const float* mask,
                           const int64_t* rng, float s, float sigma, float sigma_next, float eta, float sqrt_1m_eta2, int32_t step, int32_t B,
                           int64_t n_s, int64_t n_mask, void* stream) {
  if (!x || !v || B < 1 || n_s < 1 || n_mask < 1 || (mask && (!src || !noise)) || (!rng && sigma_next != 0.0f)) return RT_E_BADARG;
  if (!(eta > 0.0f && eta <= 1.0f) || step < 0) return RT_E_BADARG;
  if (B > 65535 || ((int64_t)B * n_s) % n_mask) return RT_E_SHAPE;
  const int64_t n4 = stochastic_vec(x, v, v_text, x_bf16, src, noise, mask, B, n_s, n_mask) ? n_s / 4 : 0;
  const auto kernel = mask ? (v_text ? stochastic_step_f32_kernel<true, true> : stochastic_step_f32_kernel<false, true>)
                           : (v_text ? stochastic_step_f32_kernel<true, false> : stochastic_step_f32_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(grid_for(n4 > 0 ? n4 : n_s, 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, (const bf16_t*)v,
                     (const bf16_t*)v_text, (bf16_t*)x_bf16, src, noise, mask, rng, s, sigma, sigma_next, eta, sqrt_1m_eta2, (uint32_t)step, n_s, n_mask, n4);
  return rt_hip_status();
}

int rt_projected_stochastic_step_f32(float* x, const void* v_uncond, const void* v_text, void* x_bf16, const float* diff, const float* partials,
                                     float s_minus_1, float eta_guidance, float tau, const float* src, const float* noise, const float* mask,
                                     const int64_t* rng, float sigma, float sigma_next, float eta, float sqrt_1m_eta2, int32_t step, int32_t B,
                                     int64_t n_s, int64_t n_mask, void* stream) {
  if (!x || !v_uncond || !v_text || !diff || !partials || B < 1 || n_s < 1 || n_mask < 1 || (mask && (!src || !noise)) ||
      (!rng && sigma_next != 0.0f))
    return RT_E_BADARG;
  if (!(eta > 0.0f && eta <= 1.0f) || step < 0) return RT_E_BADARG;
  const int64_t chunks = (n_s + RT_GUIDE_CHUNK - 1) / RT_GUIDE_CHUNK;
  if (B > 65535 || chunks > 0x7fffffff || ((int64_t)B * n_s) % n_mask) return RT_E_SHAPE;
  const int64_t n4 = stochastic_vec(x, nullptr, v_text, x_bf16, src, noise, mask, B, n_s, n_mask) && RT_ALIGNED(diff, 16) ? n_s / 4 : 0;
  const auto kernel = mask ? projected_stochastic_step_f32_kernel<true> : projected_stochastic_step_f32_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(grid_for(n4 > 0 ? n4 : n_s, 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, (const bf16_t*)v_text,
                     (bf16_t*)x_bf16, diff, partials, (int)chunks, s_minus_1, eta_guidance, tau, src, noise, mask, rng, sigma, sigma_next, eta,
                     sqrt_1m_eta2, (uint32_t)step, n_s, n_mask, n4);
  return rt_hip_status();
}

int rt_normal_fill_f32(float* out, const int64_t* rng, int32_t B, int64_t n_s, int32_t step, void* stream) {
  if (!out || !rng || B < 1 || n_s < 1 || step < 0) return RT_E_BADARG;
  if (B > 65535) return RT_E_SHAPE;
  const int64_t n4 = n_s % 4 == 0 && RT_ALIGNED(out, 16) ? n_s / 4 : 0;
  hipLaunchKernelGGL(normal_fill_f32_kernel, dim3(grid_for(n4 > 0 ? n4 : n_s, 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, out, rng,
                     (uint32_t)step, n_s, n4);
  return rt_hip_status();
}

int rt_cfg_mix(const void* v_uncond, const void* v_text, void* out, float s, int64_t n, void* stream) {
  if (!v_uncond || !v_text || !out || n < 1) return RT_E_BADARG;
  return launch_1d(cfg_mix_kernel, n, stream, (const bf16_t*)v_uncond, (const bf16_t*)v_text, (bf16_t*)out, s, n);
}

int rt_pack_latents(const void* nchw, void* packed, int32_t B, int32_t C, int32_t H2, int32_t W2, void* stream) {
  if (!nchw || !packed || B < 1 || C < 1 || H2 < 2 || W2 < 2 || H2 % 2 || W2 % 2) return RT_E_BADARG;
  const int64_t n = (int64_t)B * C * H2 * W2;
  return launch_1d(pack_latents_kernel, n, stream, (const bf16_t*)nchw, (bf16_t*)packed, B, C, H2, W2);
}

int rt_unpack_latents(const void* packed, void* nhwc, int32_t B, int32_t C, int32_t H2, int32_t W2, float inv_scale,
                      float shift, void* stream) {
  if (!packed || !nhwc || B < 1 || C < 1 || H2 < 2 || W2 < 2 || H2 % 2 || W2 % 2) return RT_E_BADARG;
  const int64_t n = (int64_t)B * C * H2 * W2;
  return launch_1d(unpack_latents_kernel, n, stream, (const bf16_t*)packed, (bf16_t*)nhwc, B, C, H2, W2, inv_scale, shift);
}

int rt_cast_f32_to_bf16(const float* x, void* y, int64_t n, void* stream) {
  if (!x || !y || n < 1) return RT_E_BADARG;
  return launch_1d(cast_f32_bf16_kernel, n, stream, x, (bf16_t*)y, n);
}
int rt_cast_bf16_to_f32(const void* x, float* y, int64_t n, void* stream) {
  if (!x || !y || n < 1) return RT_E_BADARG;
  return launch_1d(cast_bf16_f32_kernel, n, stream, (const bf16_t*)x, y, n);
}

int rt_silu_split_bf16(const float* x, void* hi, void* lo, int64_t n, int32_t apply_silu, void* stream) {
  if (!x || !hi || !lo || n < 1) return RT_E_BADARG;
  return launch_1d(silu_split_kernel, n, stream, x, (bf16_t*)hi, (bf16_t*)lo, n, apply_silu);
}

int rt_masked_accumulate(const void* x, void* y, const float* rowscale, float alpha, int32_t batch, int32_t rows,
                         int32_t D, int32_t accumulate, int32_t y_f32, void* stream) {
  if (!x || !y || batch < 1 || rows < 1 || D < 8) return RT_E_BADARG;
  if (D % 8) return RT_E_SHAPE;
  if (!RT_ALIGNED(x, 16) || !RT_ALIGNED(y, 16)) return RT_E_ALIGN;
  const int64_t n = (int64_t)batch * rows * (D / 8);
  if (y_f32) return launch_1d(masked_accumulate_f32_kernel, n, stream, (const bf16_t*)x, (float*)y, rowscale, alpha, batch, rows, D / 8, accumulate);
  return launch_1d(masked_accumulate_kernel, n, stream, (const bf16_t*)x, (bf16_t*)y, rowscale, alpha, batch, rows, D / 8, accumulate);
}

int rt_gelu_erf_bf16(const float* x, void* y, int64_t n, void* stream) {
  if (!x || !y || n < 1) return RT_E_BADARG;
  return launch_1d(gelu_erf_kernel, n, stream, x, (bf16_t*)y, n);
}

int rt_add_bf16_2d(const void* x, int64_t ldx, int64_t stride_xb, void* y, int64_t ldy, int64_t stride_yb, int32_t batch, int32_t rows,
                   int32_t D, void* stream) {
  if (!x || !y || batch < 1 || rows < 1 || D < 8 || ldx < D || ldy < D || stride_xb < 0 || stride_yb < 0) return RT_E_BADARG;
  if (D % 8) return RT_E_SHAPE;
  if (!RT_ALIGNED(x, 16) || !RT_ALIGNED(y, 16) || ldx % 8 || ldy % 8 || stride_xb % 8 || stride_yb % 8) return RT_E_ALIGN;
  return launch_1d(add_bf16_2d_kernel, (int64_t)batch * rows * (D / 8), stream, (const bf16_t*)x, ldx, stride_xb, (bf16_t*)y, ldy, stride_yb,
                   batch, rows, D / 8);
}

}  // extern "C"
