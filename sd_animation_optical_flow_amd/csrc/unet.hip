// What the reference's UNet needs beyond the convolutions, the GroupNorm of sd_ops.hip and the transformer (transformer.hip):
//
//   ofx_groupnorm_cat        ldm/modules/diffusionmodules/openaimodel.py:257-277 (`ResBlock._forward`): GroupNorm(32) + SiLU over
//                            th.cat([h, hs.pop()], dim=1) (:786; controlnet.py:54-56) and over h + emb_out[b, c] (:275-276), with
//                            neither the concatenation nor the shifted map ever written
//   ofx_emb_linear           `time_embed` (:530-534) and the `emb_layers` of every ResBlock (:220-226): SiLU + Linear on B rows
//   ofx_timestep_embedding   ldm/modules/diffusionmodules/util.py:154-174
//
// ofx_groupnorm_cat keeps the three stages of ofx_groupnorm (sd_ops.hip) and its summation order, statement by statement: with one
// dense segment and no e the two give the same bits.  The per-image term e enters in the finalize stage alone.  A slice of n pixels
// whose channel sums are (S, Q) has, for x + e, the sums
//     S' = S + n e,        Q' = Q + 2 e S + n e^2
// in f64 (e is a float, so 2 e S and n e^2 carry one f64 rounding each), and since
//     (x + e) * scale + shift = x * scale + (shift + e * scale)
// the apply stage is the one of ofx_groupnorm with a shift that was folded in f64 and rounded once.
#include "ofx_internal.h"

#include <algorithm>
#include <cmath>

namespace {

// the slicing rule of ofx_groupnorm (sd_ops.hip: gn_slices)
static inline int gnc_slices(int B) { return B >= 4 ? 64 : 256; }

// gn_partial_kernel of sd_ops.hip with two sources: float4 column c4 of the concatenation comes from x0 when 4 c4 < C0, else from x1
// (C0 % 4 == 0: a float4 never straddles the seam)
__global__ __launch_bounds__(256) void gnc_partial_kernel(const float* __restrict__ x0, int ld0, int C0, const float* __restrict__ x1, int ld1,
                                                          double* __restrict__ part, long HW, int C, int kSlices) {
    const int cg = C / 4;
    const int b = blockIdx.y, sl = blockIdx.x;
    const long per = (HW + kSlices - 1) / kSlices;
    const long beg = sl * per, end = beg + per < HW ? beg + per : HW;
    __shared__ double red[256 * 8];
    // channel groups beyond 256 threads (C > 1024) are walked in passes
    for (int c0 = 0; c0 < cg; c0 += 256) {
        const int ncg = min(256, cg - c0);
        const int rws = 256 / ncg;
        const int tc = threadIdx.x % ncg, tr = threadIdx.x / ncg;
        double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
        if (tr < rws) {
            const int ch = (c0 + tc) * 4;
            const long ld = ch < C0 ? ld0 : ld1;
            const float* base = (ch < C0 ? x0 + ch : x1 + (ch - C0)) + ((long)b * HW) * ld;
            for (long i = beg + tr; i < end; i += rws) {
                const float4 v = *reinterpret_cast<const float4*>(base + i * ld);
                s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
                q[0] += (double)v.x * v.x; q[1] += (double)v.y * v.y; q[2] += (double)v.z * v.z; q[3] += (double)v.w * v.w;
            }
        }
        for (int k = 0; k < 4; ++k) {
            red[threadIdx.x * 8 + k] = s[k];
            red[threadIdx.x * 8 + 4 + k] = q[k];
        }
        __syncthreads();
        if ((int)threadIdx.x < ncg) {
            double ts[4] = {0, 0, 0, 0}, tq[4] = {0, 0, 0, 0};
            for (int r = 0; r < rws; ++r)
                for (int k = 0; k < 4; ++k) {
                    ts[k] += red[(r * ncg + threadIdx.x) * 8 + k];
                    tq[k] += red[(r * ncg + threadIdx.x) * 8 + 4 + k];
                }
            double* o = part + (((long)b * kSlices + sl) * C + (c0 + threadIdx.x) * 4) * 2;
            for (int k = 0; k < 4; ++k) {
                o[k * 2] = ts[k];
                o[k * 2 + 1] = tq[k];
            }
        }
        __syncthreads();
    }
}

// gn_finalize_kernel of sd_ops.hip; with e, every (slice, channel) pair of sums is moved to the sums of x + e before it is added
// (header), and the shift takes e * scale.  The thread layout and the order of the additions are unchanged.
__global__ __launch_bounds__(256) void gnc_finalize_kernel(const double* __restrict__ part, const float* __restrict__ e, int lde,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ scale, float* __restrict__ shift, long HW, int C, int groups,
                                                           float eps, int kSlices) {
    __shared__ double rs[256], rq[256];
    __shared__ double gmu[256], grs[256];
    const int b = blockIdx.x;
    const int cpg = C / groups;
    const int tpg = groups >= 256 ? 1 : 256 / groups;          // threads per group
    const long per = (HW + kSlices - 1) / kSlices;
    const float* eb = e ? e + (long)b * lde : nullptr;
    for (int g0 = 0; g0 < groups; g0 += 256 / tpg) {
        const int gl = threadIdx.x / tpg, sub = threadIdx.x - gl * tpg;
        const int g = g0 + gl;
        double s = 0, q = 0;
        if (g < groups)
            for (int sl = sub; sl < kSlices; sl += tpg) {
                const double* o = part + (((long)b * kSlices + sl) * C + g * cpg) * 2;
                if (eb) {
                    const long beg = sl * per, end = beg + per < HW ? beg + per : HW;
                    const double n = end > beg ? (double)(end - beg) : 0.0;         // pixels of this slice
                    for (int c = 0; c < cpg; ++c) {
                        const double ec = (double)eb[g * cpg + c];
                        s += o[2 * c] + n * ec;
                        q += o[2 * c + 1] + 2.0 * ec * o[2 * c] + n * ec * ec;
                    }
                } else {
                    for (int c = 0; c < cpg; ++c) {
                        s += o[2 * c];
                        q += o[2 * c + 1];
                    }
                }
            }
        rs[threadIdx.x] = s;
        rq[threadIdx.x] = q;
        __syncthreads();
        if (sub == 0 && g < groups) {
            s = 0; q = 0;
            for (int k = 0; k < tpg; ++k) {
                s += rs[threadIdx.x + k];
                q += rq[threadIdx.x + k];
            }
            const double n = (double)HW * cpg;
            const double mu = s / n;
            double var = q / n - mu * mu;
            if (var < 0) var = 0;
            gmu[gl] = mu;
            grs[gl] = 1.0 / sqrt(var + (double)eps);
        }
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += 256) {
            const int g2 = c / cpg - g0;
            if (g2 >= 0 && g2 < 256 / tpg) {
                const double r = grs[g2] * (double)(gamma ? gamma[c] : 1.f);
                scale[(long)b * C + c] = (float)r;
                if (eb)
                    shift[(long)b * C + c] = (float)((double)(beta ? beta[c] : 0.f) - (gmu[g2] - (double)eb[c]) * r);
                else
                    shift[(long)b * C + c] = (float)((double)(beta ? beta[c] : 0.f) - gmu[g2] * r);
            }
        }
        __syncthreads();
    }
}

// gn_apply_kernel of sd_ops.hip reading the two segments, writing the dense concatenation
__global__ __launch_bounds__(256) void gnc_apply_kernel(const float* __restrict__ x0, int ld0, int C0, const float* __restrict__ x1, int ld1,
                                                        const float* __restrict__ scale, const float* __restrict__ shift, float* out, long HW,
                                                        int C, long total4, int silu) {
    const int cg = C / 4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % cg) * 4;
        const long row = i / cg;
        const long b = row / HW;
        const float* src = c < C0 ? x0 + row * ld0 + c : x1 + row * ld1 + (c - C0);
        const float4 v = *reinterpret_cast<const float4*>(src);
        const float4 sc = *reinterpret_cast<const float4*>(scale + b * C + c);
        const float4 sh = *reinterpret_cast<const float4*>(shift + b * C + c);
        float4 y = make_float4(fmaf(v.x, sc.x, sh.x), fmaf(v.y, sc.y, sh.y), fmaf(v.z, sc.z, sh.z), fmaf(v.w, sc.w, sh.w));
        if (silu) {
            y.x = y.x / (1.0f + expf(-y.x));
            y.y = y.y / (1.0f + expf(-y.y));
            y.z = y.z / (1.0f + expf(-y.z));
            y.w = y.w / (1.0f + expf(-y.w));
        }
        reinterpret_cast<float4*>(out)[i] = y;
    }
}

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
    return (size_t)B * gnc_slices(B) * C * 2 * sizeof(double) + (size_t)B * C * 2 * sizeof(float);
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
    hipStream_t s = (hipStream_t)stream;
    const int kSlices = gnc_slices(B);
    double* part = reinterpret_cast<double*>(scratch);
    float* scale = reinterpret_cast<float*>(part + (size_t)B * kSlices * C * 2);
    float* shift = scale + (size_t)B * C;
    {
        OfxProfScope prof("groupnorm_cat_partial", s);
        hipLaunchKernelGGL(gnc_partial_kernel, dim3(kSlices, B), dim3(256), 0, s, x0, ld0, C0, x1, ld1, part, HW, C, kSlices);
    }
    {
        OfxProfScope prof("groupnorm_cat_finalize", s);
        hipLaunchKernelGGL(gnc_finalize_kernel, dim3(B), dim3(256), 0, s, part, e, lde, gamma, beta, scale, shift, HW, C, groups, eps, kSlices);
    }
    int st = ofx_launch_status();
    if (st) return st;
    const long total4 = (long)B * HW * (C / 4);
    OfxProfScope prof("groupnorm_cat_apply", s);
    hipLaunchKernelGGL(gnc_apply_kernel, dim3((unsigned)std::min<long>((total4 + 255) / 256, 65536)), dim3(256), 0, s, x0, ld0, C0, x1, ld1, scale,
                       shift, out, HW, C, total4, silu);
    return ofx_launch_status();
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
