// The fused attention kernel templates and their launchers, shared by attn_flash.hip (the 20 instantiations on one K and one V
// tensor) and attn_flash_segs.hip (the 20 segmented-K/V instantiations of the strided addressing).  attn_flash.hip describes the
// kernels; every instantiation lives in the file that launches it, so a file compiles exactly the kernels it names.
#pragma once
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

// Segmented K/V (ofx_attention_bnhd_segs): K and V of image b are the logical concatenation of cnt[b] segments, entries
// e[first[b]] .. e[first[b] + cnt[b] - 1], each with its own pointers and row strides and the logical index `start` of its first
// key.  The table travels by value in the kernel arguments (2.2 KB): no device allocation, no lifetime rule.  The entry index of
// the walk below is wave-uniform, so entries are read with scalar loads: when a tile passes a seam (FlashSegState keeps the segment
// a tile starts in), and per row only in a tile that straddles one, where a staged row keeps the last entry whose start it reaches.
constexpr int kSegMax = 8;          // OFX_KV_MAX_SEGMENTS
constexpr int kSegEntries = 64;     // OFX_KV_MAX_ENTRIES
struct FlashSeg {
    const char* k;
    const char* v;
    int start;                      // logical index of the segment's first key
    int n;
    int ldk, ldv;                   // row strides in elements
};
struct FlashSegArgs : FlashArgs {
    FlashSeg e[kSegEntries];
    unsigned char first[kSegEntries];
    unsigned char cnt[kSegEntries];
};
// SEG: 0 = one K and one V tensor (a.k / a.v), 1 = segments of float32, 2 = segments of float16
template <int SEG> struct FlashArgsOf { typedef FlashArgs type; };
template <> struct FlashArgsOf<1> { typedef FlashSegArgs type; };
template <> struct FlashArgsOf<2> { typedef FlashSegArgs type; };

typedef _Float16 h4v __attribute__((ext_vector_type(4)));
typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f8v __attribute__((ext_vector_type(8)));

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

// Segmented instantiations only.  The segment the tile being staged starts in, held in registers (all wave-uniform: scalar
// registers) so that a tile inside one segment -- every tile but the few that straddle a seam -- addresses its rows from these
// fields as the strided kernel addresses them from its base pointer, with no table read at all; `next` is the logical index of the
// following segment's first key (INT_MAX after the last).
struct FlashSegState {
    const char* k;
    const char* v;
    int st, lk, lv, next, cur;
};

__device__ __forceinline__ void flash_seg_enter(const FlashSegArgs& a, int e0, int ne, FlashSegState& s) {
    const FlashSeg& g = a.e[e0 + s.cur];
    s.k = g.k; s.v = g.v; s.st = g.start; s.lk = g.ldk; s.lv = g.ldv;
    s.next = s.cur + 1 < ne ? a.e[e0 + s.cur + 1].start : 0x7fffffff;
}

// Once per tile and wave-uniform (tiles are staged in ascending order of k0): move to the segment that holds logical key k0 -- the
// table is read only when a seam has been passed -- and return how many of the image's segments, from that one on, the tile
// [k0, k0 + bk) can reach: 1 when it ends inside the segment.
__device__ __forceinline__ int flash_seg_tile(const FlashSegArgs& a, int e0, int ne, int k0, int bk, FlashSegState& s) {
    if (k0 >= s.next) {
        do {
            ++s.cur;
            s.next = s.cur + 1 < ne ? a.e[e0 + s.cur + 1].start : 0x7fffffff;
        } while (k0 >= s.next);
        flash_seg_enter(a, e0, ne, s);
    }
    return s.next - k0 >= bk ? 1 : ne - s.cur;
}

// The addresses (in bytes) of element `col` of logical key kk < Nk, kk >= s.st: in the state's segment when ne == 1, else in the
// last of the ne entries from it on whose first key kk reaches (a tile that straddles a seam).  ES = bytes per element.
template <int ES>
__device__ __forceinline__ void flash_seg_row(const FlashSegArgs& a, int e0, int ne, const FlashSegState& s, int kk, int col, const char*& kp,
                                              const char*& vp) {
    const char* pk = s.k;
    const char* pv = s.v;
    int st = s.st, lk = s.lk, lv = s.lv;
    for (int i = 1; i < ne; ++i) {                  // ne and the entry index are wave-uniform
        const FlashSeg& g = a.e[e0 + s.cur + i];
        if (kk >= g.start) {
            pk = g.k; pv = g.v; st = g.start; lk = g.ldk; lv = g.ldv;
        }
    }
    kp = pk + ((long)(kk - st) * lk + col) * ES;
    vp = pv + ((long)(kk - st) * lv + col) * ES;
}

// STRIDED = false: [BH, N, D] tensors, a batch-head is one contiguous run.  STRIDED = true: tokens are rows of ld floats with the
// heads side by side in a row (what a fused q|k|v projection GEMM leaves); only the global addresses differ, the arithmetic and
// its order are the same, so the two instantiations agree bit for bit.  SEG != 0 (STRIDED only): K / V rows come from the segment
// table, float32 (SEG = 1) or float16 converted exactly as they are staged (SEG = 2); the tile walk, the bias column, the ragged
// mask and the softmax use the logical key index, so the result is bit for bit that of SEG = 0 on the concatenated tensor.  SEG is
// a template parameter and every use is `if constexpr`: the SEG = 0 instantiations compile to what they were without it.
template <int D, int BK, bool STRIDED, int SEG = 0>
__global__ __launch_bounds__(256) void flash_attn_kernel(const typename FlashArgsOf<SEG>::type a) {
    static_assert(D % 8 == 0 && D <= 160, "head size");
    static_assert(SEG == 0 || STRIDED, "segments use the strided addressing");
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
    int seg0 = 0, segn = 0;                         // SEG: the image's entries, and the one the tile being staged starts in
    FlashSegState seg{};
    if constexpr (SEG != 0) {
        seg0 = a.first[img];
        segn = a.cnt[img];
        flash_seg_enter(a, seg0, segn, seg);
    }

    float4 sk[PER], sv[PER];
    auto load_tile = [&](int k0) __attribute__((always_inline)) {
        int tne = 0;                                // SEG: the entries this tile's rows choose among, from the state's on
        if constexpr (SEG != 0) tne = flash_seg_tile(a, seg0, segn, k0, BK, seg);
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int f = tid + 256 * p;
            const int key = f / (D / 4);
            const bool ok = (PER * 256 == NF4 || f < NF4) && k0 + key < a.Nk;
            if constexpr (SEG != 0) {
                // the row's segment from its logical key index; 16-byte loads of float32 rows, 8-byte loads of float16 rows
                const int c4 = f % (D / 4);
                sk[p] = make_float4(0.f, 0.f, 0.f, 0.f);
                sv[p] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok) {
                    const char *kp, *vp;
                    flash_seg_row<SEG == 1 ? 4 : 2>(a, seg0, tne, seg, k0 + key, hoff + 4 * c4, kp, vp);
                    if constexpr (SEG == 1) {
                        sk[p] = *reinterpret_cast<const float4*>(kp);
                        sv[p] = *reinterpret_cast<const float4*>(vp);
                    } else {
                        const f4v xk = __builtin_convertvector(*reinterpret_cast<const h4v*>(kp), f4v);   // exact
                        const f4v xv = __builtin_convertvector(*reinterpret_cast<const h4v*>(vp), f4v);
                        sk[p] = make_float4(xk[0], xk[1], xk[2], xk[3]);
                        sv[p] = make_float4(xv[0], xv[1], xv[2], xv[3]);
                    }
                }
            } else if constexpr (STRIDED) {
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

template <int D, int BK, bool STRIDED, int SEG = 0>
int launch_flash(const typename FlashArgsOf<SEG>::type& a, hipStream_t s) {
    constexpr int LDK = D + 4, LDV = ((D + 7) / 16) * 16 + 8;
    constexpr size_t lds = 2 * (size_t)(BK * LDK + BK * LDV + 32) * sizeof(float);
    if (lds > 65536) {                               // > 64 KB of dynamic LDS needs the opt-in (per device: set on every launch, it is cheap)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&flash_attn_kernel<D, BK, STRIDED, SEG>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((flash_attn_kernel<D, BK, STRIDED, SEG>), dim3((unsigned)(a.BH * a.qtiles)), dim3(256), lds, s, a);
    return ofx_launch_status();
}

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
// SEG as in flash_attn_kernel: float32 rows (SEG = 1) are rounded as they are staged, like a.k / a.v; float16 rows (SEG = 2) are
// staged as they are, with no second rounding -- bit for bit SEG = 0 on float32 values that round to them.
template <int D, int BK, bool STRIDED, int SEG = 0>
__global__ __launch_bounds__(256, 2) void flash_attn_f16_kernel(const typename FlashArgsOf<SEG>::type a) {
    static_assert(D % 8 == 0 && D <= 160 && BK % 32 == 0, "head size");
    static_assert(SEG == 0 || STRIDED, "segments use the strided addressing");
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

    int seg0 = 0, segn = 0;                         // SEG: the image's entries, and the one the tile being staged starts in
    FlashSegState seg{};
    if constexpr (SEG != 0) {
        seg0 = a.first[img];
        segn = a.cnt[img];
        flash_seg_enter(a, seg0, segn, seg);
    }

    h4v sk[PER], sv[PER];                           // rounded as they are staged: half the registers of the fp32 form
    auto load_tile = [&](int k0) __attribute__((always_inline)) {
        int tne = 0;                                // SEG: the entries this tile's rows choose among, from the state's on
        if constexpr (SEG != 0) tne = flash_seg_tile(a, seg0, segn, k0, BK, seg);
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int f = tid + 256 * p;
            const int key = f / (D / 4);
            const bool ok = (PER * 256 == NF4 || f < NF4) && k0 + key < a.Nk;
            float4 tk = make_float4(0.f, 0.f, 0.f, 0.f), tv = tk;
            if constexpr (SEG == 2) {
                // float16 rows: staged as they are (8-byte loads), no rounding here
                const h4v z = {0, 0, 0, 0};
                sk[p] = z;
                sv[p] = z;
                if (ok) {
                    const char *kp, *vp;
                    flash_seg_row<2>(a, seg0, tne, seg, k0 + key, hoff + 4 * (f % (D / 4)), kp, vp);
                    sk[p] = *reinterpret_cast<const h4v*>(kp);
                    sv[p] = *reinterpret_cast<const h4v*>(vp);
                }
                continue;
            } else if constexpr (SEG == 1) {
                if (ok) {
                    const char *kp, *vp;
                    flash_seg_row<4>(a, seg0, tne, seg, k0 + key, hoff + 4 * (f % (D / 4)), kp, vp);
                    tk = *reinterpret_cast<const float4*>(kp);
                    tv = *reinterpret_cast<const float4*>(vp);
                }
            } else if constexpr (STRIDED) {
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

template <int D, int BK, bool STRIDED, int SEG = 0>
int launch_flash_f16(const typename FlashArgsOf<SEG>::type& a, hipStream_t s) {
    constexpr int DP = (D + 15) / 16 * 16;
    constexpr size_t lds = 2 * (size_t)(BK * (DP + 8) + BK * f16_ldv(D)) * sizeof(_Float16);
    static_assert(lds <= 65536, "no opt-in needed");
    hipLaunchKernelGGL((flash_attn_f16_kernel<D, BK, STRIDED, SEG>), dim3((unsigned)(a.BH * a.qtiles)), dim3(256), lds, s, a);
    return ofx_launch_status();
}

}  // namespace

// The fused head sizes and the keys per K / V tile of each: the one list behind ofx_attention_flash_ok and every dispatch
#define OFX_FLASH_SIZES(X) X(40, 64) X(64, 32) X(80, 32) X(128, 32) X(160, 32)

// the fields every launch derives: the scale in base 2, the query tiles, the raster
static int flash_derive(FlashArgs& a, float scale, int precision) {
    if (precision != OFX_PREC_FP32 && precision != OFX_PREC_F16) return OFX_EINVAL;
    a.scale_log2e = scale * kLog2e;
    a.qtiles = ofx_cdiv(a.Nq, 128);
    a.xcd_grouped = (a.BH % 8 == 0) ? 1 : 0;
    if ((long)a.BH * a.qtiles > 0x7fffffffL) return OFX_EINVAL;
    return 0;
}
