// What `SpatialTransformer` (ldm/modules/attention.py:472-537) needs besides the convolution / GroupNorm / attention kernels:
//
//   ofx_layernorm            nn.LayerNorm(C) in front of each of the three sub-blocks of BasicTransformerBlock (:456-458, :465-468).
//                            One wave per row, the row held in registers (C = 1280: 20 floats per lane): the mean first, then the
//                            sum of squares of the centred values (no E[x^2] - mean^2 cancellation), both by wave reductions.
//                            float4 loads and stores, no LDS, no scratch.
//   ofx_geglu                GEGLU.forward (:54-56) after its Linear: out = a[:, :inner] * gelu(a[:, inner:]), gelu in the exact
//                            erf form F.gelu defaults to.
//   ofx_attention_bnhd_f32   the fused attention kernel (attn_flash.hip) on token rows with the heads side by side: q / k / v are
//                            read where the projection GEMM left them and the output is written where the next GEMM reads it, so
//                            MemoryEfficientCrossAttention.forward's four permute(...).contiguous() copies (:338-345, :430-435) go.
#include "ofx_internal.h"

#include <cmath>

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// NV float4 per lane cover a row of up to 256 * NV floats; lanes past the row hold zeros and store nothing
template <int NV>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* out, long ldo, int rows, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                // wave-uniform
    const int c4n = C >> 2;
    const float* xr = x + row * ldx;
    float4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c4 = lane + 64 * i;
        v[i] = c4 < c4n ? *reinterpret_cast<const float4*>(xr + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c4 = lane + 64 * i;
        v[i] = make_float4(v[i].x - mean, v[i].y - mean, v[i].z - mean, v[i].w - mean);
        if (c4 < c4n) q += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
    float* orow = out + row * ldo;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c4 = lane + 64 * i;
        if (c4 < c4n) {
            const float4 g = gamma ? *reinterpret_cast<const float4*>(gamma + 4 * c4) : make_float4(1.f, 1.f, 1.f, 1.f);
            const float4 b = beta ? *reinterpret_cast<const float4*>(beta + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(orow + 4 * c4) =
                make_float4(v[i].x * rstd * g.x + b.x, v[i].y * rstd * g.y + b.y, v[i].z * rstd * g.z + b.z, v[i].w * rstd * g.w + b.w);
        }
    }
}

template <int NV>
void launch_layernorm(const float* x, long ldx, const float* gamma, const float* beta, float* out, long ldo, int rows, int C, float eps,
                      hipStream_t s) {
    hipLaunchKernelGGL(layernorm_kernel<NV>, dim3((unsigned)ofx_cdiv(rows, 4)), dim3(256), 0, s, x, ldx, gamma, beta, out, ldo, rows, C, eps);
}

__device__ __forceinline__ float gelu_erf(float g) { return 0.5f * g * (1.0f + erff(g * 0.70710678118654752440f)); }

__global__ __launch_bounds__(256) void geglu_kernel(const float* a, long lda, float* out, long ldo, int inner4, long total4) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
        const long r = i / inner4;
        const int c4 = (int)(i - r * inner4);
        const float* ar = a + r * lda + 4 * c4;
        const float4 xv = *reinterpret_cast<const float4*>(ar);
        const float4 gv = *reinterpret_cast<const float4*>(ar + 4 * (long)inner4);
        *reinterpret_cast<float4*>(out + r * ldo + 4 * c4) =
            make_float4(xv.x * gelu_erf(gv.x), xv.y * gelu_erf(gv.y), xv.z * gelu_erf(gv.z), xv.w * gelu_erf(gv.w));
    }
}

}  // namespace

extern "C" {

int ofx_layernorm(const float* x, int ldx, const float* gamma, const float* beta, float* out, int ldo, int rows, int C, float eps,
                  void* stream) {
    OFX_REQUIRE(x && out && rows > 0 && C > 0 && C <= 4096 && ldx >= C && ldo >= C && eps >= 0.f, OFX_EINVAL);
    OFX_REQUIRE(C % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && ofx_aligned16(x) && ofx_aligned16(out) && ofx_aligned16(gamma) &&
                    ofx_aligned16(beta), OFX_EALIGN);
    hipStream_t s = (hipStream_t)stream;
    OfxProfScope prof("layernorm", s);
    const int need = ofx_cdiv(C, 256);
    if (need <= 1) launch_layernorm<1>(x, ldx, gamma, beta, out, ldo, rows, C, eps, s);
    else if (need <= 2) launch_layernorm<2>(x, ldx, gamma, beta, out, ldo, rows, C, eps, s);
    else if (need <= 3) launch_layernorm<3>(x, ldx, gamma, beta, out, ldo, rows, C, eps, s);
    else if (need <= 5) launch_layernorm<5>(x, ldx, gamma, beta, out, ldo, rows, C, eps, s);
    else if (need <= 8) launch_layernorm<8>(x, ldx, gamma, beta, out, ldo, rows, C, eps, s);
    else launch_layernorm<16>(x, ldx, gamma, beta, out, ldo, rows, C, eps, s);
    return ofx_launch_status();
}

int ofx_geglu(const float* a, int lda, float* out, int ldo, int rows, int inner, void* stream) {
    OFX_REQUIRE(a && out && rows > 0 && inner > 0 && lda >= 2 * (long)inner && ldo >= inner, OFX_EINVAL);
    OFX_REQUIRE(inner % 4 == 0 && lda % 4 == 0 && ldo % 4 == 0 && ofx_aligned16(a) && ofx_aligned16(out), OFX_EALIGN);
    hipStream_t s = (hipStream_t)stream;
    const long total4 = (long)rows * (inner / 4);
    OfxProfScope prof("geglu", s);
    hipLaunchKernelGGL(geglu_kernel, dim3((unsigned)std::min<long>((total4 + 255) / 256, 65536)), dim3(256), 0, s, a, (long)lda, out, (long)ldo,
                       inner / 4, total4);
    return ofx_launch_status();
}

// the checks of both entry points; precision is OFX_PREC_FP32 or OFX_PREC_F16 here
static int attention_bnhd_checked(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* bias, long bias_bstride,
                                  float* out, int ldo, int B, int H, int Nq, int Nk, int D, float scale, int precision, void* stream) {
    OFX_REQUIRE(q && k && v && out && B > 0 && H > 0 && Nq > 0 && Nk > 0 && ofx_attention_flash_ok(D), OFX_EINVAL);
    OFX_REQUIRE((long)B * H <= 0x7fffffffL, OFX_EINVAL);
    const long hd = (long)H * D;
    OFX_REQUIRE(ldq >= hd && ldk >= hd && ldv >= hd && ldo >= hd, OFX_EINVAL);
    OFX_REQUIRE(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldo % 4 == 0 && ofx_aligned16(q) && ofx_aligned16(k) && ofx_aligned16(v) &&
                    ofx_aligned16(out) && (uintptr_t)bias % 4 == 0, OFX_EALIGN);
    return ofx_attention_flash_bnhd_launch(q, ldq, k, ldk, v, ldv, bias, bias_bstride, out, ldo, B, H, Nq, Nk, D, scale, precision,
                                           (hipStream_t)stream);
}

int ofx_attention_bnhd_f32(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* bias, long bias_bstride,
                           float* out, int ldo, int B, int H, int Nq, int Nk, int D, float scale, void* stream) {
    return attention_bnhd_checked(q, ldq, k, ldk, v, ldv, bias, bias_bstride, out, ldo, B, H, Nq, Nk, D, scale, OFX_PREC_FP32, stream);
}

int ofx_attention_bnhd_prec(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* bias, long bias_bstride,
                            float* out, int ldo, int B, int H, int Nq, int Nk, int D, float scale, int precision, void* stream) {
    OFX_REQUIRE(precision == OFX_PREC_FP32 || precision == OFX_PREC_F16, OFX_EINVAL);
    return attention_bnhd_checked(q, ldq, k, ldk, v, ldv, bias, bias_bstride, out, ldo, B, H, Nq, Nk, D, scale, precision, stream);
}

int ofx_attention_bnhd_segs(const float* q, int ldq, const ofx_kv_segment* segs, const int* seg_counts, int kv_type, const float* bias,
                            long bias_bstride, float* out, int ldo, int B, int H, int Nq, int D, float scale, int precision, void* stream) {
    OFX_REQUIRE(precision == OFX_PREC_FP32 || precision == OFX_PREC_F16, OFX_EINVAL);
    OFX_REQUIRE(kv_type == OFX_KV_F32 || kv_type == OFX_KV_F16, OFX_EINVAL);
    OFX_REQUIRE(q && segs && seg_counts && out && B > 0 && H > 0 && Nq > 0 && ofx_attention_flash_ok(D), OFX_EINVAL);
    OFX_REQUIRE((long)B * H <= 0x7fffffffL && B <= OFX_KV_MAX_ENTRIES, OFX_EINVAL);
    const long hd = (long)H * D;
    OFX_REQUIRE(ldq >= hd && ldo >= hd, OFX_EINVAL);
    OFX_REQUIRE(ldq % 4 == 0 && ldo % 4 == 0 && ofx_aligned16(q) && ofx_aligned16(out) && (uintptr_t)bias % 4 == 0, OFX_EALIGN);
    // float32 rows are staged with 16-byte loads, half rows with 8-byte loads: 4 elements either way
    const uintptr_t amask = kv_type == OFX_KV_F32 ? 15u : 7u;
    long Nk = -1;
    int at = 0;
    for (int b = 0; b < B; ++b) {
        const int cnt = seg_counts[b];
        OFX_REQUIRE(cnt >= 1 && cnt <= OFX_KV_MAX_SEGMENTS && at + cnt <= OFX_KV_MAX_ENTRIES, OFX_EINVAL);
        long total = 0;
        for (int i = 0; i < cnt; ++i, ++at) {
            const ofx_kv_segment& g = segs[at];
            OFX_REQUIRE(g.k && g.v && g.n > 0 && g.ldk >= hd && g.ldv >= hd, OFX_EINVAL);
            OFX_REQUIRE(g.ldk % 4 == 0 && g.ldv % 4 == 0 && ((uintptr_t)g.k & amask) == 0 && ((uintptr_t)g.v & amask) == 0, OFX_EINVAL);
            total += g.n;
        }
        OFX_REQUIRE(total <= 0x7fffffffL && (Nk < 0 || total == Nk), OFX_EINVAL);
        Nk = total;
    }
    return ofx_attention_flash_segs_launch(q, ldq, segs, seg_counts, kv_type, bias, bias_bstride, out, ldo, B, H, Nq, (int)Nk, D, scale,
                                           precision, (hipStream_t)stream);
}

}  // extern "C"
