// What the CLIP text encoder (`FrozenCLIPEmbedder` through hack.py:23-70, transformers' CLIPTextModel) needs besides the
// LayerNorm / GEMM / attention kernels `SpatialTransformer` is built from:
//
//   ofx_clip_embed    CLIPTextEmbeddings.forward: out[r] = token_embedding[ids[r]] + position_embedding[r % T].  A row gather and
//                     one fp32 addition per element, so the bits are torch's.  An id outside [0, vocab) reads nothing and its row
//                     comes out as quiet NaNs.
//   ofx_quick_gelu    the activation between the MLP's two Linears (hidden_act = "quick_gelu"): x * sigmoid(1.702 x), written
//                     x / (1 + expf(-1.702f x)) with the accurate expf and an IEEE division.
//
// Both are bandwidth- and launch-bound: one float4 per lane per trip, consecutive lanes on consecutive float4 of a row (a wave
// reads and writes 1 KiB runs), a grid-stride loop over rows * (C / 4) float4 with 64-bit indices, so any row count is covered by at
// most 65536 workgroups.  No LDS, no scratch.
#include "ofx_internal.h"

#include <algorithm>
#include <cmath>

namespace {

__global__ __launch_bounds__(256) void clip_embed_kernel(const int32_t* __restrict__ ids, const float* __restrict__ tok,
                                                         const float* __restrict__ pos, float* __restrict__ out, long ldo, int T, int c4n,
                                                         int vocab, long total4) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
        const long r = i / c4n;
        const int c4 = (int)(i - r * c4n);
        const int id = ids[r];
        float4 v;
        if (id >= 0 && id < vocab) {
            const float4 t = *reinterpret_cast<const float4*>(tok + ((long)id * c4n + c4) * 4);
            const float4 p = *reinterpret_cast<const float4*>(pos + ((r % T) * c4n + c4) * 4);
            v = make_float4(t.x + p.x, t.y + p.y, t.z + p.z, t.w + p.w);
        } else {                                            // no read: a visible wrong answer, not a clamp
            const float q = __builtin_nanf("");
            v = make_float4(q, q, q, q);
        }
        *reinterpret_cast<float4*>(out + r * ldo + 4 * c4) = v;
    }
}

// finite for every finite x: expf overflows to +inf below x = -52.1 and x / inf = -0; above, expf underflows to 0 and x / 1 = x
__device__ __forceinline__ float quick_gelu(float x) { return x / (1.0f + expf(-(1.702f * x))); }

// out may be x itself: an element is read and written by the same lane
__global__ __launch_bounds__(256) void quick_gelu_kernel(const float* x, long ldx, float* out, long ldo, int n4, long total4) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
        const long r = i / n4;
        const int c4 = (int)(i - r * n4);
        const float4 v = *reinterpret_cast<const float4*>(x + r * ldx + 4 * c4);
        *reinterpret_cast<float4*>(out + r * ldo + 4 * c4) = make_float4(quick_gelu(v.x), quick_gelu(v.y), quick_gelu(v.z), quick_gelu(v.w));
    }
}

unsigned grid_for(long total4) { return (unsigned)std::min<long>((total4 + 255) / 256, 65536); }

}  // namespace

extern "C" {

int ofx_clip_embed(const int32_t* ids, const float* tok, const float* pos, float* out, int ldo, long rows, int T, int C, int vocab,
                   void* stream) {
    OFX_REQUIRE(ids && tok && pos && out && rows >= 0 && T > 0 && C > 0 && vocab > 0 && ldo >= C, OFX_EINVAL);
    OFX_REQUIRE(C % 4 == 0 && ldo % 4 == 0 && (uintptr_t)ids % 4 == 0 && ofx_aligned16(tok) && ofx_aligned16(pos) && ofx_aligned16(out),
                OFX_EALIGN);
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const long total4 = rows * (C / 4);
    OfxProfScope prof("clip_embed", s);
    hipLaunchKernelGGL(clip_embed_kernel, dim3(grid_for(total4)), dim3(256), 0, s, ids, tok, pos, out, (long)ldo, T, C / 4, vocab, total4);
    return ofx_launch_status();
}

int ofx_quick_gelu(const float* x, int ldx, float* out, int ldo, long rows, int n, void* stream) {
    OFX_REQUIRE(x && out && rows >= 0 && n > 0 && ldx >= n && ldo >= n, OFX_EINVAL);
    OFX_REQUIRE(n % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && ofx_aligned16(x) && ofx_aligned16(out), OFX_EALIGN);
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const long total4 = rows * (n / 4);
    OfxProfScope prof("quick_gelu", s);
    hipLaunchKernelGGL(quick_gelu_kernel, dim3(grid_for(total4)), dim3(256), 0, s, x, (long)ldx, out, (long)ldo, n / 4, total4);
    return ofx_launch_status();
}

}  // extern "C"
