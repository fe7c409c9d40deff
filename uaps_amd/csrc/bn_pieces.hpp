// Pieces of the BatchNorm(train) + LeakyReLU kernels that more than one file uses: norm_act.hip's own passes and the encoder glue of
// enc_glue.hip (the gradient fan-in that forms the backward sums while it still holds the summed gradient in registers, the apply
// pass that also pools).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace uaps {
constexpr int kBnThreads = 256;    // threads per block of every streaming BatchNorm kernel
constexpr int kBnChunk = 4096;     // floats per block: 4 float4 per thread

__device__ __forceinline__ float2 block_sum2(float a, float b) {
    __shared__ float2 red[kBnThreads / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = make_float2(a, b);
    __syncthreads();
    float2 r = red[0];
#pragma unroll
    for (int w = 1; w < kBnThreads / 64; ++w) { r.x += red[w].x; r.y += red[w].y; }
    return r;
}

// d(pre-activation) from d(out): dropout mask/scale, then LeakyReLU slope chosen by the sign of the
// recomputed BN output z (torch: grad * (z > 0 ? 1 : slope)).
__device__ __forceinline__ float dpre(float dout, float yv, float mu, float sc, float sh, float slope) {
    const float z = (yv - mu) * sc + sh;
    return z > 0.f ? dout : dout * slope;
}

// enc_glue.hip: bn_apply_kernel<true, false> that also writes MaxPool2d(2) of its result (uaps_bn_apply_pool_support(H, W) holds,
// y / out / pooled 16-byte and idx 4-byte aligned); grid and block as every apply pass: (chunks, planes) x kBnThreads
void launch_bn_apply_pool(const float* y, float* out, float* pooled, uint8_t* idx, int B, int C, int H, int W, const float* mean,
                          const float* coef, float slope, int Bg, float* amax, hipStream_t stream);
}  // namespace uaps
