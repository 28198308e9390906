// Fused attention for the UNet's head sizes: out = softmax(q k^T * scale + bias) v without the
// score matrix ever leaving the CU -- the form `xformers.ops.memory_efficient_attention` has at
// ldm/modules/attention.py:314,426 (16384 tokens x 8 heads at 1024x1024: 8.6 GB of scores per image in the unfused form).
//
// Written for the 32x32x2 fp32 matrix-core instruction, transposed so that nothing has to move between lanes:
//
//   S^T = K Q^T     A operand = K tile rows from LDS (b128 reads: a lane takes 4 consecutive d of its key),
//                   B operand = the wave's 32 queries, pre-scaled by scale * log2(e), held in registers for the whole key loop.
//                   The accumulator of lane (c = lane % 32, h = lane / 32) holds S^T[key = 8i + 4h + j][query = c]:
//                   one query per lane column, so the row maximum / row sum of the softmax are IN-LANE reductions over 16
//                   registers plus one exchange with lane ^ 32.
//   O^T += V^T P^T  the k index of this product is the key; the instruction wants, from half h of the wave, the key pair
//                   member h -- and register 4i + j of half h already holds key 8i + 4h + j.  So MFMA number 4i + j takes P^T
//                   straight from the accumulator register it was computed in, with the V operand read as
//                   V[key = 8i + 4h + j][d = c]: no shuffle, no LDS round trip for P.
//
// Online softmax in base 2 (v_exp_f32): m = running maximum, l = running sum per lane half (the halves share m, their partial
// sums are added once at the end), O rescaled only when some query's maximum moved (wave-uniform branch; exact, the factor
// is 1.0 otherwise).  K / V tiles of 64 (32 for d > 40) keys are double-buffered in LDS behind register-staged global loads.
// Everything is fp32; summation order differs from the unfused path, results agree to rounding.
//
// flash_attn_f16_kernel is the opt-in OFX_PREC_F16 form of the same skeleton (ofx_attention_prec / ofx_attention_bnhd_prec): 128
// queries per workgroup, 4 waves of 32 queries, double-buffered K / V tiles behind register-staged global loads, the same raster,
// bias forms, base-2 online softmax, wave-uniform rescale and m_use rule.  Its arithmetic contract:
//   operands   q, k, v are fp32 in memory; each element is rounded to fp16 ONCE, round-to-nearest-even (the _Float16 vector
//              conversion, v_cvt_pk_f16_f32 -- not the truncating pkrtz form), as it is staged.  q is rounded UNSCALED.  Magnitudes
//              beyond 65504 become infinities (as under torch.autocast); subnormals are kept, the matrix core multiplies them.
//   S^T = K Q^T  on v_mfma_f32_32x32x16_f16, fp32 accumulate: A = 8 halves of a K row from LDS (one b128 read), B = the wave's
//              queries in registers.  D = 40 runs as 48: the 8 pad columns are zeros in the Q fragment and are written as zeros
//              into both LDS buffers once before the loop (no tile store touches them; stale LDS times zero could be NaN).
//   logit      x = fma(S, scale * log2e, bias * log2e) on the fp32 score: scale and the fp32 bias never pass through fp16.
//   softmax    maximum, v_exp_f32, the running sum l, the O accumulators, the rescale and the final 1 / l are fp32; l sums the
//              fp32 probabilities BEFORE they are rounded.
//   O^T += V^T P^T  P is rounded to fp16 (RNE) straight from the accumulator registers: registers 8s .. 8s+7 converted pairwise are
//              the B fragment of k-step s, whose element j in lane half h is key 16s + 8(j>>2) + 4h + (j&3) of the block.  V is
//              staged ROW-MAJOR as halves ([key][LDV], the same coalesced float4 -> 4 halves store as K) and the A fragment is two
//              ds_read_b64_tr_b16 per k-step and 32-row tile: the hardware transpose hands lane (c, h) V[16s + 8a + 4h + e][32tt + c]
//              in element e of read a -- exactly that permuted key order.  Chosen over a transposed image because staging stays
//              one b64 store per float4 (a transposed image needs four b16 stores) and K and V share one store pattern.  Banks
//              (a 32-lane half reads 4 key rows x 16 dwords): LDV / 2 dwords = 16 * odd puts the four rows on four disjoint 16-bank
//              runs, conflict-free; LDK = DP + 8 halves = 4 * odd dwords, conflict-free for b128 reads as in the fp32 kernel.
//              LDV >= 32 * DT, so tiles with d >= D read inside their own row (rows of O^T that are never stored).
//   Two workgroups per CU (__launch_bounds__(256, 2)): one wave's softmax runs under the other's MFMAs.
//
// The two kernels share the raster (flash_raster) and nothing else on purpose: the bias / ragged mask, the online-softmax step and
// the output epilogue stay written out in both.  Forceinline helpers for any of them change the compiled instruction stream, and the
// softmax step as a helper moves register allocation in 12 of the 20 instantiations (flash_attn_kernel<40, 64, false>: 160 -> 176
// registers, occupancy 3 -> 2).  The raster helper leaves all 20 instruction-identical.
#include "ofx_internal.h"

#include <cmath>

namespace {

typedef float v16f __attribute__((ext_vector_type(16)));

struct FlashArgs {
    const float* q;
    const float* k;
    const float* v;
    const float* bias;   // [Nq, Nk] per batch-head (bias_bs = Nq * Nk) or shared (bias_bs = 0); may be null
    float* out;
    long bias_bs;
    int BH, Nq, Nk;
    float scale_log2e;
    int qtiles;
    int xcd_grouped;
    // STRIDED instantiation only (ofx_attention_bnhd_f32): element (b, n, h, d) at p[(b * N + n) * ld + h * D + d], bh = b * H + h
    int H;
    int ldq, ldk, ldv, ldo;
};

constexpr float kLog2e = 1.4426950408889634f;

// the workgroup's batch-head and tile of 128 queries (both kernels)
__device__ __forceinline__ void flash_raster(const FlashArgs& a, int& bh, int& qt) {
    if (a.xcd_grouped) {
        // consecutive workgroup ids go round the 8 XCDs: give every XCD whole batch-heads so that their K / V stay in its L2
        const int id = blockIdx.x, xcd = id & 7, slot = id >> 3;
        bh = (slot / a.qtiles) * 8 + xcd;
        qt = slot % a.qtiles;
    } else {
        bh = blockIdx.x / a.qtiles;
        qt = blockIdx.x % a.qtiles;
    }
}

// STRIDED = false: [BH, N, D] tensors, a batch-head is one contiguous run.  STRIDED = true: tokens are rows of ld floats with the
// heads side by side in a row (what a fused q|k|v projection GEMM leaves); only the global addresses differ, the arithmetic and
// its order are the same, so the two instantiations agree bit for bit.
template <int D, int BK, bool STRIDED>
__global__ __launch_bounds__(256) void flash_attn_kernel(const FlashArgs a) {
    static_assert(D % 8 == 0 && D <= 160, "head size");
    constexpr int DQ = D / 8;                       // groups of 8 along d: each wave half takes 4 of them
    constexpr int DT = (D + 31) / 32;               // 32-row tiles of O^T
    constexpr int LDK = D + 4;                      // K row stride (floats): conflict-free b128 fragment reads
    constexpr int LDV = ((D + 7) / 16) * 16 + 8;    // V row stride: = 8 mod 16, so keys 4 apart sit 32 banks apart
    constexpr int KT = BK * LDK;
    constexpr int VT = BK * LDV + 32;               // slack: the last d tile reads past D (into rows that are never stored)
    constexpr int NF4 = BK * D / 4;                 // float4 per tensor per tile
    constexpr int PER = (NF4 + 255) / 256;
    extern __shared__ float smem[];                 // [2][KT + VT]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 31, h = lane >> 5;

    int bh, qt;
    flash_raster(a, bh, qt);
    const int qrow = qt * 128 + wave * 32 + c;
    const bool qok = qrow < a.Nq;

    // the wave's queries, scaled: lane (c, h) keeps q[qrow][8m + 4h + 0..3]
    // STRIDED: image and head of this batch-head, and the head's column offset in a token row
    const int img = STRIDED ? bh / a.H : 0;
    const int hoff = STRIDED ? (bh % a.H) * D : 0;
    float4 qreg[DQ];
    {
        const float* qp = STRIDED ? a.q + ((long)img * a.Nq + (qok ? qrow : 0)) * a.ldq + hoff + 4 * h
                                  : a.q + ((long)bh * a.Nq + (qok ? qrow : 0)) * D + 4 * h;
#pragma unroll
        for (int m = 0; m < DQ; ++m) {
            float4 t = qok ? *reinterpret_cast<const float4*>(qp + 8 * m) : make_float4(0.f, 0.f, 0.f, 0.f);
            qreg[m] = make_float4(t.x * a.scale_log2e, t.y * a.scale_log2e, t.z * a.scale_log2e, t.w * a.scale_log2e);
        }
    }

    const float* kg = STRIDED ? a.k + (long)img * a.Nk * a.ldk + hoff : a.k + (long)bh * a.Nk * D;
    const float* vg = STRIDED ? a.v + (long)img * a.Nk * a.ldv + hoff : a.v + (long)bh * a.Nk * D;
    const float* bg = a.bias ? a.bias + (long)bh * a.bias_bs + (long)(qok ? qrow : 0) * a.Nk : nullptr;

    float4 sk[PER], sv[PER];
    auto load_tile = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int f = tid + 256 * p;
            const int key = f / (D / 4);
            const bool ok = (PER * 256 == NF4 || f < NF4) && k0 + key < a.Nk;
            if constexpr (STRIDED) {
                // a key is D contiguous floats (D / 4 consecutive lanes read one 4 * D-byte run), keys are ld floats apart
                const int c4 = f % (D / 4);
                sk[p] = ok ? *reinterpret_cast<const float4*>(kg + (long)(k0 + key) * a.ldk + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
                sv[p] = ok ? *reinterpret_cast<const float4*>(vg + (long)(k0 + key) * a.ldv + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                // a tile is one contiguous run of BK * D floats
                sk[p] = ok ? *reinterpret_cast<const float4*>(kg + (long)k0 * D + 4 * f) : make_float4(0.f, 0.f, 0.f, 0.f);
                sv[p] = ok ? *reinterpret_cast<const float4*>(vg + (long)k0 * D + 4 * f) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };
    auto store_tile = [&](float* buf) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int f = tid + 256 * p;
            if (PER * 256 == NF4 || f < NF4) {
                const int key = f / (D / 4), c4 = f % (D / 4);
                *reinterpret_cast<float4*>(buf + key * LDK + 4 * c4) = sk[p];
                *reinterpret_cast<float4*>(buf + KT + key * LDV + 4 * c4) = sv[p];
            }
        }
    };

    v16f o[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[t][e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    const int nt = (a.Nk + BK - 1) / BK;
    load_tile(0);
    store_tile(smem);
    __syncthreads();

    for (int t = 0; t < nt; ++t) {
        const float* buf = smem + (t & 1) * (KT + VT);
        if (t + 1 < nt) load_tile((t + 1) * BK);
        const int k0 = t * BK;
#pragma unroll
        for (int kb = 0; kb < BK / 32; ++kb) {
            const int kbase = k0 + kb * 32;
            if (kbase >= a.Nk) break;                       // wave-uniform
            v16f s;
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = 0.f;
            const float* kr = buf + (kb * 32 + c) * LDK + 4 * h;
#pragma unroll
            for (int m = 0; m < DQ; ++m) {
                const float4 kf = *reinterpret_cast<const float4*>(kr + 8 * m);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qreg[m].x, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qreg[m].y, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qreg[m].z, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qreg[m].w, s, 0, 0, 0);
            }
            if (bg) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int key = kbase + 8 * i + 4 * h + j;
                        if (key < a.Nk) s[4 * i + j] += bg[key] * kLog2e;
                    }
            }
            if (kbase + 32 > a.Nk) {                        // ragged last block: keys past the end take no weight
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (kbase + 8 * i + 4 * h + j >= a.Nk) s[4 * i + j] = -INFINITY;
            }
            float mx = s[0];
#pragma unroll
            for (int e = 1; e < 16; ++e) mx = fmaxf(mx, s[e]);
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float m_new = fmaxf(m_run, mx);
            const float m_use = m_new == -INFINITY ? 0.f : m_new;       // a row whose every key so far is masked out
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);  // exp2(-inf) = 0 on the first block
            float ps = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                s[e] = __builtin_amdgcn_exp2f(s[e] - m_use);
                ps += s[e];
            }
            l_run = l_run * alpha + ps;
            if (__builtin_amdgcn_ballot_w64(m_new != m_run) != 0) {
#pragma unroll
                for (int tt = 0; tt < DT; ++tt)
#pragma unroll
                    for (int e = 0; e < 16; ++e) o[tt][e] *= alpha;
            }
            m_run = m_new;
            const float* vr = buf + KT + (kb * 32 + 4 * h) * LDV + c;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int tt = 0; tt < DT; ++tt)
                        o[tt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[(8 * i + j) * LDV + 32 * tt], s[4 * i + j], o[tt], 0, 0, 0);
                }
        }
        if (t + 1 < nt) store_tile(smem + ((t + 1) & 1) * (KT + VT));
        __syncthreads();
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv = 1.0f / l_tot;
    if (qok) {
        float* op = STRIDED ? a.out + ((long)img * a.Nq + qrow) * a.ldo + hoff : a.out + ((long)bh * a.Nq + qrow) * D;
#pragma unroll
        for (int tt = 0; tt < DT; ++tt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int d0 = 32 * tt + 8 * i + 4 * h;
                if (d0 < D)
                    *reinterpret_cast<float4*>(op + d0) =
                        make_float4(o[tt][4 * i] * inv, o[tt][4 * i + 1] * inv, o[tt][4 * i + 2] * inv, o[tt][4 * i + 3] * inv);
            }
    }
}

template <int D, int BK, bool STRIDED>
int launch_flash(const FlashArgs& a, hipStream_t s) {
    constexpr int LDK = D + 4, LDV = ((D + 7) / 16) * 16 + 8;
    constexpr size_t lds = 2 * (size_t)(BK * LDK + BK * LDV + 32) * sizeof(float);
    if (lds > 65536) {                               // > 64 KB of dynamic LDS needs the opt-in (per device: set on every launch, it is cheap)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&flash_attn_kernel<D, BK, STRIDED>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((flash_attn_kernel<D, BK, STRIDED>), dim3((unsigned)(a.BH * a.qtiles)), dim3(256), lds, s, a);
    return ofx_launch_status();
}

typedef _Float16 h4v __attribute__((ext_vector_type(4)));
typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f8v __attribute__((ext_vector_type(8)));

__device__ __forceinline__ h4v f16_round4(const float4 t) {       // v_cvt_pk_f16_f32 x 2: round to nearest even
    const f4v x = {t.x, t.y, t.z, t.w};
    return __builtin_convertvector(x, h4v);
}

// ds_read_b64_tr_b16: needs EXEC all ones (every call site is wave-uniform control flow in a 256-thread workgroup)
__device__ __forceinline__ h4v lds_read_tr16(const _Float16* p) {
    typedef __fp16 raw4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
    typedef __attribute__((address_space(3))) raw4 lds_raw4;
    const raw4 r = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_raw4*)(p));
    return __builtin_bit_cast(h4v, r);
}

constexpr int f16_ldv(int D) { return D <= 96 ? 96 : 160; }       // halves; LDV / 2 = 16 * odd dwords and LDV >= 32 * ceil(D / 32)

// OFX_PREC_F16 (header): the same skeleton on v_mfma_f32_32x32x16_f16.  FlashArgs is shared; scale_log2e multiplies the fp32 score.
template <int D, int BK, bool STRIDED>
__global__ __launch_bounds__(256, 2) void flash_attn_f16_kernel(const FlashArgs a) {
    static_assert(D % 8 == 0 && D <= 160 && BK % 32 == 0, "head size");
    constexpr int DP = (D + 15) / 16 * 16;          // the contraction length of the scores: D = 40 runs as 48
    constexpr int KS = DP / 16;                     // k-steps of S^T = K Q^T
    constexpr int DT = (D + 31) / 32;               // 32-row tiles of O^T
    constexpr int LDK = DP + 8;                     // K row stride (halves): 4 * odd dwords, conflict-free b128 fragment reads
    constexpr int LDV = f16_ldv(D);                 // V row stride (halves)
    static_assert(LDV >= 32 * DT && (LDV / 2) % 32 == 16, "V row stride");
    constexpr int KT = BK * LDK;
    constexpr int VT = BK * LDV;
    constexpr int NF4 = BK * D / 4;                 // float4 per tensor per tile
    constexpr int PER = (NF4 + 255) / 256;
    extern __shared__ __attribute__((aligned(16))) _Float16 smem16[];   // [2][KT + VT]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 31, h = lane >> 5;

    int bh, qt;
    flash_raster(a, bh, qt);
    const int qrow = qt * 128 + wave * 32 + c;
    const bool qok = qrow < a.Nq;

    // the wave's queries, rounded unscaled: lane (c, h) keeps q[qrow][16s + 8h + 0..7]; columns at and past D are zeros
    const int img = STRIDED ? bh / a.H : 0;
    const int hoff = STRIDED ? (bh % a.H) * D : 0;
    h8v qf[KS];
    {
        const float* qp = STRIDED ? a.q + ((long)img * a.Nq + (qok ? qrow : 0)) * a.ldq + hoff + 8 * h
                                  : a.q + ((long)bh * a.Nq + (qok ? qrow : 0)) * D + 8 * h;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const bool in = qok && (16 * s + 8 * h < D);
            const float4 t0 = in ? *reinterpret_cast<const float4*>(qp + 16 * s) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 t1 = in ? *reinterpret_cast<const float4*>(qp + 16 * s + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            const h4v lo = f16_round4(t0), hi = f16_round4(t1);
            qf[s] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        }
    }

    const float* kg = STRIDED ? a.k + (long)img * a.Nk * a.ldk + hoff : a.k + (long)bh * a.Nk * D;
    const float* vg = STRIDED ? a.v + (long)img * a.Nk * a.ldv + hoff : a.v + (long)bh * a.Nk * D;
    const float* bg = a.bias ? a.bias + (long)bh * a.bias_bs + (long)(qok ? qrow : 0) * a.Nk : nullptr;

    h4v sk[PER], sv[PER];                           // rounded as they are staged: half the registers of the fp32 form
    auto load_tile = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int f = tid + 256 * p;
            const int key = f / (D / 4);
            const bool ok = (PER * 256 == NF4 || f < NF4) && k0 + key < a.Nk;
            float4 tk = make_float4(0.f, 0.f, 0.f, 0.f), tv = tk;
            if constexpr (STRIDED) {
                const int c4 = f % (D / 4);
                if (ok) {
                    tk = *reinterpret_cast<const float4*>(kg + (long)(k0 + key) * a.ldk + 4 * c4);
                    tv = *reinterpret_cast<const float4*>(vg + (long)(k0 + key) * a.ldv + 4 * c4);
                }
            } else {
                if (ok) {
                    tk = *reinterpret_cast<const float4*>(kg + (long)k0 * D + 4 * f);
                    tv = *reinterpret_cast<const float4*>(vg + (long)k0 * D + 4 * f);
                }
            }
            sk[p] = f16_round4(tk);
            sv[p] = f16_round4(tv);
        }
    };
    auto store_tile = [&](_Float16* buf) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int f = tid + 256 * p;
            if (PER * 256 == NF4 || f < NF4) {
                const int key = f / (D / 4), c4 = f % (D / 4);
                *reinterpret_cast<h4v*>(buf + key * LDK + 4 * c4) = sk[p];
                *reinterpret_cast<h4v*>(buf + KT + key * LDV + 4 * c4) = sv[p];
            }
        }
    };

    if constexpr (DP != D) {
        // the pad columns D .. DP-1 of every K row of both buffers: zeros, written once (store_tile stays below column D)
        static_assert(DP - D == 8, "pad");
        for (int r = tid; r < 2 * BK; r += 256) {
            const h8v z = {0, 0, 0, 0, 0, 0, 0, 0};
            *reinterpret_cast<h8v*>(smem16 + (r / BK) * (KT + VT) + (r % BK) * LDK + D) = z;
        }
    }

    v16f o[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[t][e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    const int nt = (a.Nk + BK - 1) / BK;
    load_tile(0);
    store_tile(smem16);
    __syncthreads();

    // transposed V read (ds_read_b64_tr_b16): in its 16-lane group, lane 4q + p supplies the address of row q, columns 4p .. 4p+3 of a
    // 4-key x 16-column block and receives column (lane % 16) of the four keys.  Group g = lane / 16 takes columns 16 (g & 1) ..,
    // keys 4h .. 4h+3 (h = g >> 1) of each 8-key run.
    const int tr_off = (4 * h + ((lane >> 2) & 3)) * LDV + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);

    for (int t = 0; t < nt; ++t) {
        const _Float16* buf = smem16 + (t & 1) * (KT + VT);
        if (t + 1 < nt) load_tile((t + 1) * BK);
        const int k0 = t * BK;
#pragma unroll
        for (int kb = 0; kb < BK / 32; ++kb) {
            const int kbase = k0 + kb * 32;
            if (kbase >= a.Nk) break;                       // wave-uniform
            v16f s;
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = 0.f;
            const _Float16* kr = buf + (kb * 32 + c) * LDK + 8 * h;
#pragma unroll
            for (int m = 0; m < KS; ++m) {
                const h8v kf = *reinterpret_cast<const h8v*>(kr + 16 * m);
                s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[m], s, 0, 0, 0);
            }
            if (bg) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int key = kbase + 8 * i + 4 * h + j;
                        const float b = key < a.Nk ? bg[key] * kLog2e : 0.f;
                        s[4 * i + j] = __builtin_fmaf(s[4 * i + j], a.scale_log2e, b);
                    }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) s[e] *= a.scale_log2e;
            }
            if (kbase + 32 > a.Nk) {                        // ragged last block: keys past the end take no weight
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (kbase + 8 * i + 4 * h + j >= a.Nk) s[4 * i + j] = -INFINITY;
            }
            float mx = s[0];
#pragma unroll
            for (int e = 1; e < 16; ++e) mx = fmaxf(mx, s[e]);
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float m_new = fmaxf(m_run, mx);
            const float m_use = m_new == -INFINITY ? 0.f : m_new;       // a row whose every key so far is masked out
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);  // exp2(-inf) = 0 on the first block
            float ps = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                s[e] = __builtin_amdgcn_exp2f(s[e] - m_use);
                ps += s[e];                                             // l sums the fp32 probabilities, before they are rounded
            }
            l_run = l_run * alpha + ps;
            if (__builtin_amdgcn_ballot_w64(m_new != m_run) != 0) {
#pragma unroll
                for (int tt = 0; tt < DT; ++tt)
#pragma unroll
                    for (int e = 0; e < 16; ++e) o[tt][e] *= alpha;
            }
            m_run = m_new;
            const _Float16* vr = buf + KT + kb * 32 * LDV + tr_off;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const f8v p8 = {s[8 * ks], s[8 * ks + 1], s[8 * ks + 2], s[8 * ks + 3], s[8 * ks + 4], s[8 * ks + 5], s[8 * ks + 6], s[8 * ks + 7]};
                const h8v pf = __builtin_convertvector(p8, h8v);        // P rounded to fp16 (RNE), still in its accumulator lanes
#pragma unroll
                for (int tt = 0; tt < DT; ++tt) {
                    const h4v v0 = lds_read_tr16(vr + (16 * ks) * LDV + 32 * tt);
                    const h4v v1 = lds_read_tr16(vr + (16 * ks + 8) * LDV + 32 * tt);
                    const h8v vf = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
                    o[tt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, o[tt], 0, 0, 0);
                }
            }
        }
        if (t + 1 < nt) store_tile(smem16 + ((t + 1) & 1) * (KT + VT));
        __syncthreads();
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv = 1.0f / l_tot;
    if (qok) {
        float* op = STRIDED ? a.out + ((long)img * a.Nq + qrow) * a.ldo + hoff : a.out + ((long)bh * a.Nq + qrow) * D;
#pragma unroll
        for (int tt = 0; tt < DT; ++tt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int d0 = 32 * tt + 8 * i + 4 * h;
                if (d0 < D)
                    *reinterpret_cast<float4*>(op + d0) =
                        make_float4(o[tt][4 * i] * inv, o[tt][4 * i + 1] * inv, o[tt][4 * i + 2] * inv, o[tt][4 * i + 3] * inv);
            }
    }
}

template <int D, int BK, bool STRIDED>
int launch_flash_f16(const FlashArgs& a, hipStream_t s) {
    constexpr int DP = (D + 15) / 16 * 16;
    constexpr size_t lds = 2 * (size_t)(BK * (DP + 8) + BK * f16_ldv(D)) * sizeof(_Float16);
    static_assert(lds <= 65536, "no opt-in needed");
    hipLaunchKernelGGL((flash_attn_f16_kernel<D, BK, STRIDED>), dim3((unsigned)(a.BH * a.qtiles)), dim3(256), lds, s, a);
    return ofx_launch_status();
}

}  // namespace

// The fused head sizes and the keys per K / V tile of each: the one list behind ofx_attention_flash_ok and every dispatch
#define OFX_FLASH_SIZES(X) X(40, 64) X(64, 32) X(80, 32) X(128, 32) X(160, 32)

bool ofx_attention_flash_ok(int D) {
#define X(d, bk) if (D == d) return true;
    OFX_FLASH_SIZES(X)
#undef X
    return false;
}

// the launch of head size D from the list, for one kernel family and one addressing
template <bool F16, bool STRIDED>
static int flash_launch_d(const FlashArgs& a, int D, hipStream_t s) {
    switch (D) {
#define X(d, bk)                                                            \
    case d:                                                                 \
        if constexpr (F16) return launch_flash_f16<d, bk, STRIDED>(a, s);   \
        else return launch_flash<d, bk, STRIDED>(a, s);
        OFX_FLASH_SIZES(X)
#undef X
    }
    return OFX_EINVAL;
}

static int flash_dispatch(FlashArgs& a, int D, float scale, bool strided, int precision, hipStream_t s) {
    if (precision != OFX_PREC_FP32 && precision != OFX_PREC_F16) return OFX_EINVAL;
    a.scale_log2e = scale * kLog2e;
    a.qtiles = ofx_cdiv(a.Nq, 128);
    a.xcd_grouped = (a.BH % 8 == 0) ? 1 : 0;
    if ((long)a.BH * a.qtiles > 0x7fffffffL) return OFX_EINVAL;
    if (precision == OFX_PREC_F16) {
        OfxProfScope prof(strided ? "attn_flash_bnhd_f16" : "attn_flash_f16", s);
        prof.flops(4.0 * a.BH * (double)a.Nq * a.Nk * D);
        return strided ? flash_launch_d<true, true>(a, D, s) : flash_launch_d<true, false>(a, D, s);
    }
    OfxProfScope prof(strided ? "attn_flash_bnhd" : "attn_flash", s);
    prof.flops(4.0 * a.BH * (double)a.Nq * a.Nk * D);
    return strided ? flash_launch_d<false, true>(a, D, s) : flash_launch_d<false, false>(a, D, s);
}

int ofx_attention_flash_launch(const float* q, const float* k, const float* v, const float* bias, long bias_bstride, float* out, int BH, int Nq,
                               int Nk, int D, float scale, int precision, hipStream_t s) {
    FlashArgs a{};
    a.q = q; a.k = k; a.v = v; a.bias = bias; a.out = out;
    a.bias_bs = bias_bstride;
    a.BH = BH; a.Nq = Nq; a.Nk = Nk;
    return flash_dispatch(a, D, scale, false, precision, s);
}

int ofx_attention_flash_bnhd_launch(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* bias,
                                    long bias_bstride, float* out, int ldo, int B, int H, int Nq, int Nk, int D, float scale, int precision, hipStream_t s) {
    FlashArgs a{};
    a.q = q; a.k = k; a.v = v; a.bias = bias; a.out = out;
    a.bias_bs = bias_bstride;
    a.BH = B * H; a.Nq = Nq; a.Nk = Nk;
    a.H = H; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    return flash_dispatch(a, D, scale, true, precision, s);
}
