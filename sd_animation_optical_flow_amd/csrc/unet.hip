// What the reference's UNet needs beyond the convolutions, the GroupNorm of sd_ops.hip and the transformer (transformer.hip):
//
//   ofx_groupnorm_cat        ldm/modules/diffusionmodules/openaimodel.py:257-277 (`ResBlock._forward`): GroupNorm(32) + SiLU over
//                            th.cat([h, hs.pop()], dim=1) (:786; controlnet.py:54-56) and over h + emb_out[b, c] (:275-276), with
//                            neither the concatenation nor the shifted map ever written
//   ofx_emb_linear           `time_embed` (:530-534) and the `emb_layers` of every ResBlock (:220-226): SiLU + Linear on B rows
//   ofx_timestep_embedding   ldm/modules/diffusionmodules/util.py:154-174
//
// ofx_groupnorm_cat validates here and runs the GroupNorm kernels of sd_ops.hip (ofx_groupnorm_launch), the ones ofx_groupnorm runs:
// with one dense segment and no e the two entry points launch the same kernels on the same arguments.
#include "ofx_internal.h"

#include <algorithm>
#include <cmath>

namespace {

// ---- ofx_emb_linear ------------------------------------------------------------------------------------------------------------
constexpr int EL_ROWS = 16;         // rows (B) at most
constexpr int EL_LDS = 8192;        // floats of LDS for the rows: K is walked in chunks of EL_LDS / B floats per row (a multiple of 256)
constexpr int EL_CPW = 2;           // output columns per wave
constexpr int EL_COLS = 4 * EL_CPW; // per workgroup of four waves

// One wave per output column (EL_CPW of them in turn).  Lane l owns float4 l, l + 64, ... of every chunk of a weight row and adds
// its products in that order, k ascending, one fused multiply-add each; the 64 lane sums are then added by a butterfly (xor 32, 16,
// .., 1), the bias last: the order is fixed by (K, B) alone.
__global__ __launch_bounds__(256) void emb_linear_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ out, int ldo, int B, int K, int N,
                                                         int silu_in) {
    __shared__ float rows[EL_LDS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int kc = (EL_LDS / B) / 256 * 256;                   // floats per row and chunk
    float acc[EL_CPW][EL_ROWS];
#pragma unroll
    for (int j = 0; j < EL_CPW; ++j)
#pragma unroll
        for (int b = 0; b < EL_ROWS; ++b) acc[j][b] = 0.f;
    for (int k0 = 0; k0 < K; k0 += kc) {
        const int kn = min(kc, K - k0);                        // a multiple of 4
        const int kn4 = kn / 4;
        __syncthreads();
        for (int i = threadIdx.x; i < B * kn4; i += 256) {
            const int b = i / kn4, k4 = i - b * kn4;
            float4 v = *reinterpret_cast<const float4*>(x + (long)b * ldx + k0 + k4 * 4);
            if (silu_in) {
                v.x = v.x / (1.0f + expf(-v.x));
                v.y = v.y / (1.0f + expf(-v.y));
                v.z = v.z / (1.0f + expf(-v.z));
                v.w = v.w / (1.0f + expf(-v.w));
            }
            *reinterpret_cast<float4*>(rows + b * kc + k4 * 4) = v;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < EL_CPW; ++j) {
            const int n = blockIdx.x * EL_COLS + j * 4 + wave;
            if (n >= N) continue;                              // uniform per wave
            const float* wr = w + (long)n * K + k0;
            for (int k4 = lane; k4 < kn4; k4 += 64) {
                const float4 wv = *reinterpret_cast<const float4*>(wr + k4 * 4);
#pragma unroll
                for (int b = 0; b < EL_ROWS; ++b)
                    if (b < B) {
                        const float4 xv = *reinterpret_cast<const float4*>(rows + b * kc + k4 * 4);
                        float a = acc[j][b];
                        a = fmaf(xv.x, wv.x, a);
                        a = fmaf(xv.y, wv.y, a);
                        a = fmaf(xv.z, wv.z, a);
                        a = fmaf(xv.w, wv.w, a);
                        acc[j][b] = a;
                    }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < EL_CPW; ++j) {
        const int n = blockIdx.x * EL_COLS + j * 4 + wave;
        if (n >= N) continue;
        const float bn = bias ? bias[n] : 0.f;
#pragma unroll
        for (int b = 0; b < EL_ROWS; ++b)
            if (b < B) {
                float a = acc[j][b];
                for (int m = 32; m > 0; m >>= 1) a += __shfl_xor(a, m, 64);
                if (lane == 0) out[(long)b * ldo + n] = a + bn;
            }
    }
}

// ---- ofx_timestep_embedding -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void timestep_embedding_kernel(const float* __restrict__ t, const float* __restrict__ freqs,
                                                                 float* __restrict__ out, int dim) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= dim) return;
    const int half = dim / 2;
    float v = 0.f;                                             // the zero column of an odd dim (util.py:170-171)
    if (j < 2 * half) {
        const float a = __fmul_rn(t[b], freqs[j < half ? j : j - half]);     // args = timesteps[:, None].float() * freqs[None] (:168)
        v = j < half ? cosf(a) : sinf(a);
    }
    out[(long)b * dim + j] = v;
}

// [p, p + n floats) and [q, q + m floats) share an address
static inline bool overlaps(const float* p, size_t n, const float* q, size_t m) { return p < q + m && q < p + n; }

}  // namespace

extern "C" {

size_t ofx_groupnorm_cat_scratch_bytes(int B, int C) {
    if (B <= 0 || C <= 0) return 0;
    return ofx_groupnorm_scratch_bytes(B, C);
}

int ofx_groupnorm_cat(const float* x0, int ld0, int C0, const float* x1, int ld1, int C1, const float* e, int lde, const float* gamma,
                      const float* beta, float* out, void* scratch, size_t scratch_bytes, int B, long HW, int groups, float eps, int silu,
                      void* stream) {
    OFX_REQUIRE(x0 && out && scratch && B > 0 && B <= 65535 && HW > 0 && C0 > 0 && C1 >= 0 && groups > 0, OFX_EINVAL);
    OFX_REQUIRE((x1 != nullptr) == (C1 > 0), OFX_EINVAL);
    const long Cl = (long)C0 + C1;
    OFX_REQUIRE(Cl < (1L << 30) && Cl % groups == 0 && ld0 >= C0 && (!x1 || ld1 >= C1) && (!e || lde >= Cl), OFX_EINVAL);
    const int C = (int)Cl;
    OFX_REQUIRE(C0 % 4 == 0 && C1 % 4 == 0 && ld0 % 4 == 0 && (!x1 || ld1 % 4 == 0), OFX_EALIGN);
    OFX_REQUIRE(ofx_aligned16(x0) && ofx_aligned16(x1) && ofx_aligned16(e) && ofx_aligned16(out) && ofx_aligned16(scratch), OFX_EALIGN);
    OFX_REQUIRE(scratch_bytes >= ofx_groupnorm_cat_scratch_bytes(B, C), OFX_ENOMEM);
    // the apply stage reads a float4 and writes the same float4 of a dense single segment: only then may out be x0
    const size_t rows = (size_t)B * (size_t)HW;
    const bool in_place = out == x0 && C1 == 0 && ld0 == C0;
    OFX_REQUIRE(in_place || !overlaps(out, rows * C, x0, (rows - 1) * ld0 + C0), OFX_EINVAL);
    OFX_REQUIRE(!x1 || !overlaps(out, rows * C, x1, (rows - 1) * ld1 + C1), OFX_EINVAL);
    static const char* const scope[3] = {"groupnorm_cat_partial", "groupnorm_cat_finalize", "groupnorm_cat_apply"};
    return ofx_groupnorm_launch(x0, ld0, C0, x1, ld1, C1, e, lde, gamma, beta, out, scratch, B, HW, groups, eps, silu, scope, (hipStream_t)stream);
}

int ofx_emb_linear(const float* x, int ldx, const float* w, const float* bias, float* out, int ldo, int B, int K, int N, int silu_in,
                   void* stream) {
    OFX_REQUIRE(x && w && out && B > 0 && B <= EL_ROWS && K > 0 && N > 0 && ldx >= K && ldo >= N, OFX_EINVAL);
    OFX_REQUIRE(K % 4 == 0 && ldx % 4 == 0 && ofx_aligned16(x) && ofx_aligned16(w), OFX_EALIGN);
    hipStream_t s = (hipStream_t)stream;
    OfxProfScope prof("emb_linear", s);
    prof.flops(2.0 * B * (double)K * N);
    hipLaunchKernelGGL(emb_linear_kernel, dim3(ofx_cdiv(N, EL_COLS)), dim3(256), 0, s, x, ldx, w, bias, out, ldo, B, K, N, silu_in);
    return ofx_launch_status();
}

int ofx_timestep_embedding(const float* t, const float* freqs, float* out, int B, int dim, void* stream) {
    OFX_REQUIRE(t && out && B > 0 && B <= 65535 && dim > 0 && (freqs || dim < 2), OFX_EINVAL);
    hipStream_t s = (hipStream_t)stream;
    OfxProfScope prof("timestep_embedding", s);
    hipLaunchKernelGGL(timestep_embedding_kernel, dim3(ofx_cdiv(dim, 256), B), dim3(256), 0, s, t, freqs, out, dim);
    return ofx_launch_status();
}

}  // extern "C"
