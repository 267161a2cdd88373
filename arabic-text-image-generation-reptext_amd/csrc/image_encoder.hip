// CLIP vision encoder (image_encoder.py): the patch embedding's im2col. The attention of its layers is attention_small_head.hip; every
// other step runs on the kernels the text encoders use.
#include "rt_common.h"

namespace {

// One thread per 8 output columns (16 bytes) of one patch row.
template <bool F32>
__global__ __launch_bounds__(256) void patchify_nchw_kernel(const void* __restrict__ x, bf16_t* __restrict__ out, int B, int G, int p, int Kp) {
  const int chunks = Kp >> 3;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * G * G * chunks) return;
  const int c8 = (int)(idx % chunks) * 8;
  const int64_t prow = idx / chunks;               // b·G² + gy·G + gx
  const int gx = (int)(prow % G), gy = (int)((prow / G) % G), b = (int)(prow / ((int64_t)G * G));
  const int pp = p * p, side = G * p;
  float f[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int col = c8 + i;
    f[i] = 0.f;
    if (col < 3 * pp) {
      const int c = col / pp, rem = col - c * pp, dy = rem / p, dx = rem - dy * p;
      const int64_t at = (((int64_t)b * 3 + c) * side + (gy * p + dy)) * side + (gx * p + dx);
      f[i] = F32 ? static_cast<const float*>(x)[at] : bf16_to_f32(static_cast<const bf16_t*>(x)[at]);
    }
  }
  *reinterpret_cast<u32x4*>(out + prow * Kp + c8) =
      u32x4{pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7])};
}

}  // namespace

extern "C" int rt_patchify_nchw(const void* x, int32_t x_f32, void* out, int32_t B, int32_t G, int32_t p, int32_t Kp, void* stream) {
  if (!x || !out || B < 1 || G < 1 || p < 1) return RT_E_BADARG;
  if (p > 1024 || G > 4096) return RT_E_SHAPE;     // keeps the index arithmetic below inside int
  if (Kp < 3 * p * p) return RT_E_BADARG;
  if (Kp % 64 || !RT_ALIGNED(out, 16) || !RT_ALIGNED(x, x_f32 ? 4 : 2)) return RT_E_ALIGN;
  const int64_t threads = (int64_t)B * G * G * (Kp / 8);
  if (threads > ((int64_t)1 << 31) - 256 || (int64_t)B * 3 * G * p * G * p >= ((int64_t)1 << 40)) return RT_E_SHAPE;
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  const hipStream_t st = (hipStream_t)stream;
  if (x_f32)
    hipLaunchKernelGGL((patchify_nchw_kernel<true>), grid, block, 0, st, x, (bf16_t*)out, B, G, p, Kp);
  else
    hipLaunchKernelGGL((patchify_nchw_kernel<false>), grid, block, 0, st, x, (bf16_t*)out, B, G, p, Kp);
  return rt_hip_status();
}
