// Fused Winograd convolutions on the fp32 matrix cores of gfx950.
//
// For the stride-1 3x3 "same" layers (the update block's convc2, conv, flow_head.conv1, convf2 and mask.0 at 1/8 resolution; the
// encoders' residual stages at 1/2 - 1/8, with their fused instance norm, residual merge and epilogue statistics) and the SepConvGRU's
// per-iteration 1x5 / 5x1 layers (gru.zr1 / q1, gru.zr2 / q2, 256 input channels) the direct halo-patch kernel of conv.hip runs at
// ~0.9 of the fp32 MFMA peak, so the only way to take real time off them is to execute fewer multiplies:
//
//   F(2x2, 3x3):  Y = A^T [ (G g G^T) (.) (B^T d B) ] A   2x2 outputs from a 4x4 input tile, 16 point products: 4 multiplies per
//                                                          output instead of 9
//   F(4, 5):      y = A^T [ (G g) (.) (B^T d) ]           4 outputs from 8 inputs, points {0, 1, -1, 2, -2, 1/2, -1/2, inf}, 8 point
//                                                          products: 2 multiplies per output instead of 5
//   F(4x4, 3x3):  the 2D form over {0, 1, -1, 2, -2, inf}   4x4 outputs from a 6x6 input tile, 36 point products: 2.25 multiplies
//                                                          per output, with an operand (ofx_conv_desc.wino4_w) and an error
//                                                          class of its own
//   (Lavin & Gray, "Fast Algorithms for Convolutional Neural Networks", 2016; Toom-Cook)
//
// Three algorithms, eighteen kernels (six fused-option or epilogue variants each), and one host section behind the kernels: a
// table with a row per algorithm (kAlgs: patch, tile arithmetic, operand, grid gate, what it admits, its kernels), and on it the
// two entries the launcher knows -- ofx_conv_wino_choose, the pure rule "which route, if any, takes this descriptor", and
// ofx_conv_wino_launch.  Nothing outside this file names an algorithm.
//
// Everything between the input and the output stays on chip -- the unfused form (transformed input and output through HBM) costs as
// much traffic as it saves multiplies ("Winograd").  F(4x4, 3x3) is described at its kernels (Halo44, below);
// F(2x2, 3x3) and F(4, 5) share one scaffold:
//   * a workgroup owns one 8x16-pixel output patch -- 32 tiles of 2x2, 1x4 (1x5 layers, along W) or 4x1 (5x1 layers, along H) --
//     and 64 (2D) or 128 (1D) output channels;
//   * per 16-channel slab the input halo is staged in LDS once (buffer descriptors return the zero padding);
//   * per transform point the GEMM [32 tiles x 16 channels] x [16 channels x 32 outputs] runs on v_mfma_f32_32x32x2_f32.  2D: wave w
//     owns the four points (w, 0..3) of the 4x4 grid and 64 outputs; 1D: wave w owns all 8 points and 32 outputs;
//   * input transform -- additions and constant scalings.  1D: every thread transforms one (tile, channel pair) and writes the
//     transformed values to LDS, where the waves read their A fragments (each wave needs all 8 points).  2D: a wave's row of the
//     point grid needs two rows of the tile's window only, so each lane forms its own A operands in registers straight from the
//     halo (wino3x3_slabs): no transformed tile in LDS, the halo double-buffered instead, one barrier per slab;
//   * the pre-transformed weights U (host, float64, one rounding: ofx_wino_conv_weight / ofx_wino15_conv_weight) are stored in the
//     MFMA's B-operand lane order, so every wave loads its own 1 KB fragments straight into registers with fully contiguous loads,
//     one slab ahead (1D, 64 registers) or one 8-channel step ahead (2D, 32 registers);
//   * output side, 2D: each wave folds its four points along the transform's column (A^T from the right), the partial rows meet in
//     LDS, and the row fold (A^T from the left) feeds the plain epilogue (scale / shift, ReLU, strided store).  1D: a lane holds the
//     8 point values of each of its (tile, channel) elements, so A^T runs in registers and the epilogue starts straight from them:
//     plain (with addend) or the two GRU gate epilogues with the semantics of igemm_kernel (conv.hip): z = sigmoid -> aux_z,
//     r * h -> aux_rh; h = (1 - z) h + z tanh(.) in place.
#include "ofx_internal.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

namespace {

constexpr int kWBK = 16;                    // channels per slab
// transformed tile row stride 20 floats: conflict-free ds_read_b128 A fragments (as the direct kernel's LDK)
constexpr int kLDV = kWBK + 4;
constexpr int kOOB = 0x7FFFFFF0;

// Input halo of an 8x16 output patch: W x H pixels from (y0 + Y0, x0 + X0); pixel `pix` (row-major) is staged at float at(pix).
template <int W_, int H_, int Y0, int X0> struct HaloGeom {
    static constexpr int W = W_, H = H_, y_org = Y0, x_org = X0;
    static constexpr int pix = W * H;                       // 180 / 160 / 192
    static constexpr int items = pix * (kWBK / 4);          // float4 pieces per slab: 720 / 640 / 768
    static constexpr int slots = (items + 255) / 256;       // per thread: 3
};
// F(4, 5): a pixel stride that puts a half-wave's transform reads in disjoint banks: 1x5, 8 x 20 at 20 (four tiles 4 pixels apart,
// 16 floats each); 5x1, 12 x 16 at 16 (four tiles 1 pixel apart).
template <bool VERT> struct Halo15 : HaloGeom<VERT ? 16 : 20, VERT ? 12 : 8, VERT ? -2 : 0, VERT ? 0 : -2> {
    static constexpr int ldh = VERT ? 16 : 20;
    static constexpr int floats = Halo15::pix * ldh;        // 3200 / 3072
    __device__ static int at(int pix) { return pix * ldh; }
};
// F(2x2, 3x3), 10 x 18: the pixels (x, x + 1), x even, are 32 contiguous floats, pairs 36 floats apart, rows 336.  Both accesses
// of the slab loop are then free of bank conflicts (tools/lds_bank_model.py, profiles/r13_lds_bank_model.txt): the staging
// ds_write_b128 (groups of 8 lanes = one pixel pair = 32 banks) and the operand ds_read_b128 (groups of 16 lanes = four runs of four
// tiles, two pixels apart along a row, from all four tile rows: 16 float4 in 16 different bank quads).
struct Halo3x3 : HaloGeom<18, 10, -1, -1> {
    static constexpr int lpair = 36, lrow = 336;
    static constexpr int floats = H * lrow;                 // 3360
    __device__ static int at(int y, int x) { return y * lrow + (x >> 1) * lpair + (x & 1) * 16; }
    __device__ static int at(int pix) { return at(pix / W, pix % W); }
};

// The argument block of all eighteen kernels (host: wino_args fills it from a descriptor and a row of kAlgs)
struct WinoK {
    const float* in0;
    const float* in1;
    const float* u;          // ofx_wino_conv_weight / ofx_wino15_conv_weight / ofx_wino44_conv_weight layout, by algorithm
    const float* scale;
    const float* shift;
    const float* addend;     // F(4, 5) only, as the GRU pointers below
    const float* res;        // the 3x3 algorithms only: residual merge relu(y + res)
    const float* nmean;      // the 3x3 algorithms only: relu((x - mean) * rstd) on the operand, [B][c0]
    const float* nrstd;
    float* stats;            // the 3x3 algorithms only: per-patch (sum, sum of squares) of every output channel, [B][tpi][Cout][2]
    float* out;
    float* aux_z;
    float* aux_rh;
    float* aux_h;
    int ld0, c0, ld1, cin, ldo, ldadd, ldh, ldres;
    int H, W, Cout, act;
    int nblk;                // output blocks of 64 (3x3) or 128 (F(4, 5)) channels
    int nb32;                // 32-channel blocks of u
    int tpr, tpi, mtiles;    // patches (8x16; F(4x4, 3x3): 16x32) per image row / per image, patches in all
    int bytes0, bytes1, bytesu;
    float alpha;
    int vec4;                // F(4x4, 3x3): out, scale, shift and res are 16-byte aligned, ldo and ldres multiples of 4 floats
};

// Output block nb of image pb's patch at (y0, x0)
struct Patch {
    int nb, pb, y0, x0;
};

// the XCD remap of conv.hip: the output blocks of one patch run back to back on one XCD (shared halo in its L2)
template <int PH = 8, int PW = 16> __device__ __forceinline__ Patch wino_patch(const WinoK& p) {
    const int nblk = p.mtiles * p.nblk;
    const int bid = blockIdx.x;
    const int q8 = nblk >> 3, r8 = nblk & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int L = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
    const int nb = L % p.nblk, mt = L / p.nblk;
    const int pb = mt / p.tpi;
    const int trem = mt - pb * p.tpi;
    const int py = trem / p.tpr;
    return {nb, pb, py * PH, (trem - py * p.tpr) * PW};
}

typedef int v4i __attribute__((ext_vector_type(4)));

// Halo staging: item i = tid + 256 k = (pixel i / 4, float4 slot i % 4) of a slab, pixels row-major over the halo.
// issue(cb) starts the loads of slab cb into registers (buffer descriptors return the zero padding), store(Hs) puts them into the
// halo buffer at Hs.  NORM: the operand is relu((x - mean) * rstd) of image pt.pb (single segment), applied as the halo is stored;
// the zero padding stays zero.
template <class HALO, bool NORM> struct HaloStage {
    const WinoK& p;
    const int pb, tid;
    const float* in1s;
    int bytes1s;
    int hpix[HALO::slots];
    unsigned hok = 0;
    int hq;                          // byte offset of this thread's float4 slot (256 % 4 == 0: the same for every k)
    struct Regs {                    // a slab in flight
        float4 pa[HALO::slots];
        float4 pmu, prs;             // NORM: mean / rstd of this thread's four channels
    } own;

    __device__ __forceinline__ HaloStage(const WinoK& p_, const Patch& pt, int tid_) : p(p_), pb(pt.pb), tid(tid_) {
        in1s = p.in1 ? p.in1 : p.in0;
        bytes1s = p.in1 ? p.bytes1 : p.bytes0;
#pragma unroll
        for (int k = 0; k < HALO::slots; ++k) {
            const int i = tid + 256 * k;
            const int pix = i >> 2;
            const int hy = pix / HALO::W, hx = pix - hy * HALO::W;
            const int gy = pt.y0 + HALO::y_org + hy, gx = pt.x0 + HALO::x_org + hx;
            const bool ok = i < HALO::items && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
            hpix[k] = ok ? (pt.pb * p.H + gy) * p.W + gx : 0;
            hok |= (ok ? 1u : 0u) << k;
        }
        hq = (tid & 3) * 16;
    }
    __device__ __forceinline__ void issue(int cb) { issue(cb, own); }
    __device__ __forceinline__ void store(float* Hs) const { store(Hs, own); }
    __device__ __forceinline__ void issue(int cb, Regs& r) {
        const int c = cb * kWBK;
        const bool s0 = c < p.c0;    // wave-uniform
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(s0 ? p.in0 : in1s), (short)0, s0 ? p.bytes0 : bytes1s, 0x00020000);
        const int so = (s0 ? c : c - p.c0) * 4;
        const int ldb = (s0 ? p.ld0 : p.ld1) * 4;
#pragma unroll
        for (int k = 0; k < HALO::slots; ++k) {
            const int vo = ((hok >> k) & 1u) ? hpix[k] * ldb + hq : kOOB;
            v4i t = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, so, 0);
            r.pa[k] = *reinterpret_cast<float4*>(&t);
        }
        if constexpr (NORM) {
            const long at = (long)pb * p.c0 + c + (tid & 3) * 4;
            r.pmu = *reinterpret_cast<const float4*>(p.nmean + at);
            r.prs = *reinterpret_cast<const float4*>(p.nrstd + at);
        }
    }
    __device__ __forceinline__ void store(float* Hs, const Regs& r) const {
#pragma unroll
        for (int k = 0; k < HALO::slots; ++k) {
            const int i = tid + 256 * k;
            if (HALO::slots * 256 > HALO::items && k == HALO::slots - 1 && i >= HALO::items) break;
            float4 v = r.pa[k];
            if constexpr (NORM) {   // as the direct kernel's a_commit (conv.hip): padding is applied to the normalised map
                v.x = fmaxf((v.x - r.pmu.x) * r.prs.x, 0.f);
                v.y = fmaxf((v.y - r.pmu.y) * r.prs.y, 0.f);
                v.z = fmaxf((v.z - r.pmu.z) * r.prs.z, 0.f);
                v.w = fmaxf((v.w - r.pmu.w) * r.prs.w, 0.f);
                if (!((hok >> k) & 1u)) v = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            *reinterpret_cast<float4*>(&Hs[HALO::at(i >> 2) + (i & 3) * 4]) = v;
        }
    }
};

// The pre-transformed weights: point pt, 32-channel block blk, 8-channel chunk c8 -> one contiguous 1 KB fragment, 16 bytes per lane
struct WinoU {
    const __amdgpu_buffer_rsrc_t rs;
    const int nb32, c8n, wlane;
    __device__ __forceinline__ WinoU(const WinoK& p, int lane)
        : rs(__builtin_amdgcn_make_buffer_rsrc((void*)p.u, (short)0, p.bytesu, 0x00020000)), nb32(p.nb32), c8n(p.cin >> 3), wlane(lane * 16) {}
    __device__ __forceinline__ float4 load(int pt, int blk, int c8) const {
        const int so = ((pt * nb32 + blk) * c8n + c8) * 1024;   // scalar
        v4i t = __builtin_amdgcn_raw_buffer_load_b128(rs, wlane, so, 0);
        return *reinterpret_cast<float4*>(&t);
    }
};

template <int P, int NT> __device__ __forceinline__ void wino_zero(f32x16 (&acc)[P][NT]) {
#pragma unroll
    for (int q = 0; q < P; ++q)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[q][nt][e] = 0.f;
}

// One 8-channel step of a point's product: A = a (tile lane & 31, channels 4 (lane >> 5) + 0..3 of the step), B = b
__device__ __forceinline__ void wino_mfma4(f32x16& acc, const float4& a, const float4& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
}

// The staged slab pipeline (F(4, 5)).  ALG is the algorithm's policy: its halo geometry ALG::HALO; the wave's share of the products,
// P transform points from ALG::pt0(wave) on and NT 32-channel blocks of u from ALG::blk0(nb, wave) on; and its input transform,
// built from (Hs, Vs, tid, wave), whose call transforms the calling thread's (tile, channel pair) from the halo in Hs into Vs
// ([point][tile][channel] at row stride kLDV).  The wave's point-wise products accumulate into acc, weights one slab ahead in
// registers: each fragment is reloaded straight behind the four MFMAs that consumed it and the scheduler is held to that
// (sched_group_barrier, as in wino3x3_slabs), so a load has 60 MFMAs and the next slab's staging to arrive in.  Every halo issue
// precedes the weight loads it shares the queue with (prologue: halo, then the fragments in the order of their use; loop: the
// next halo ahead of the products), so the wait in front of the LDS store is a counted one that leaves the weights in flight.
// The A operands are read two fragments (8 MFMAs) ahead.  tests/test_wino15_isa_schedule.py holds the compiled loop to this.
// It shares the halo geometry, the patch remap and the operand order with wino3x3_slabs but spells its staging and weight loads
// out: routed through HaloStage / WinoU the compiler scheduled the 5x1 kernels 1.5-4 % slower
// (profiles/r13_wino_rows_kernel_stats.txt).
template <class ALG>
__device__ __forceinline__ void wino_slabs_staged(const WinoK& p, const Patch& pt, float* Hs, float* Vs, int tid, int wave,
                                           f32x16 (&acc)[ALG::P][ALG::NT]) {
    using HALO = typename ALG::HALO;
    constexpr int P = ALG::P, NT = ALG::NT;
    const int lane = tid & 63;

    // ---- halo staging: item i = (pixel i / 4, float4 slot i % 4) of the slab, pixels row-major over the halo
    const float* in1s = p.in1 ? p.in1 : p.in0;
    const int bytes1s = p.in1 ? p.bytes1 : p.bytes0;
    int hpix[HALO::slots];
    unsigned hok = 0;
#pragma unroll
    for (int k = 0; k < HALO::slots; ++k) {
        const int i = tid + 256 * k;
        const int pix = i >> 2;
        const int hy = pix / HALO::W, hx = pix - hy * HALO::W;
        const int gy = pt.y0 + HALO::y_org + hy, gx = pt.x0 + HALO::x_org + hx;
        const bool ok = i < HALO::items && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
        hpix[k] = ok ? (pt.pb * p.H + gy) * p.W + gx : 0;
        hok |= (ok ? 1u : 0u) << k;
    }
    const int hq = (tid & 3) * 16;   // byte offset of this thread's float4 slot (256 % 4 == 0: the same for every k)
    float4 pa[HALO::slots];
    auto a_issue = [&](int cb) __attribute__((always_inline)) {
        const int c = cb * kWBK;
        const bool s0 = c < p.c0;    // wave-uniform
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(s0 ? p.in0 : in1s), (short)0, s0 ? p.bytes0 : bytes1s, 0x00020000);
        const int so = (s0 ? c : c - p.c0) * 4;
        const int ldb = (s0 ? p.ld0 : p.ld1) * 4;
#pragma unroll
        for (int k = 0; k < HALO::slots; ++k) {
            const int vo = ((hok >> k) & 1u) ? hpix[k] * ldb + hq : kOOB;
            v4i t = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, so, 0);
            pa[k] = *reinterpret_cast<float4*>(&t);
        }
    };

    // ---- weights: point pt0 + q, 32-channel block blk0 + nt, 8-channel chunk 2 cb + ks -> one contiguous 1 KB fragment
    const __amdgpu_buffer_rsrc_t rsu = __builtin_amdgcn_make_buffer_rsrc((void*)p.u, (short)0, p.bytesu, 0x00020000);
    const int c8n = p.cin >> 3;
    const int wlane = lane * 16;
    const int pt0 = ALG::pt0(wave), blk0 = ALG::blk0(pt.nb, wave);
    float4 wr[P][NT][2];
    auto w_issue = [&](int q, int ks, int cb) __attribute__((always_inline)) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int so = (((pt0 + q) * p.nb32 + blk0 + nt) * c8n + 2 * cb + ks) * 1024;   // scalar
            v4i t = __builtin_amdgcn_raw_buffer_load_b128(rsu, wlane, so, 0);
            wr[q][nt][ks] = *reinterpret_cast<float4*>(&t);
        }
    };

#pragma unroll
    for (int q = 0; q < P; ++q)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[q][nt][e] = 0.f;

    const ALG xf(Hs, Vs, tid, wave);
    // A fragment: tile = lane & 31, channels 8 ks + 4 (lane >> 5) + 0..3 (the k order the weights are stored in)
    const float* const afrag = Vs + (pt0 * 32 + (lane & 31)) * kLDV + 4 * (lane >> 5);

    auto a_read = [&](int i) __attribute__((always_inline)) {
        return *reinterpret_cast<const float4*>(afrag + (i >> 1) * 32 * kLDV + 8 * (i & 1));
    };

    const int CB = p.cin / kWBK;
    a_issue(0);
    // the first slab's fragments in the order of their use, and kept in it: vmcnt retires in issue order, so a fragment that the
    // scheduler moved behind its successors would be waited for together with all of them at every trip of the loop
#pragma unroll
    for (int q = 0; q < P; ++q)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            w_issue(q, ks, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    for (int cb = 0; cb < CB; ++cb) {
        const int nx = cb + 1 < CB ? cb + 1 : cb;   // the last slab re-issues itself: no branch, loads stay in bounds
#pragma unroll
        for (int k = 0; k < HALO::slots; ++k) {
            const int i = tid + 256 * k;
            if (HALO::slots * 256 > HALO::items && k == HALO::slots - 1 && i >= HALO::items) break;
            float4 v = pa[k];
            *reinterpret_cast<float4*>(&Hs[HALO::at(i >> 2) + (i & 3) * 4]) = v;
        }
        __syncthreads();
        xf();
        __syncthreads();
        a_issue(nx);   // the next slab's halo lands during this slab's products (issued here, not live across the transform)
        // ... and is issued ahead of them: left free, the scheduler sinks these loads below most of the MFMAs, and the next slab's
        // LDS store then waits for them (profiles/r09_wino_shared_ab.txt)
        __builtin_amdgcn_sched_barrier(0);
        // fragment i = (point i / 2, 8-channel step i % 2); its A operand is read two fragments (8 MFMAs) ahead
        float4 a[2 * P];
        a[0] = a_read(0);
        a[1] = a_read(1);
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
        for (int i = 0; i < 2 * P; ++i) {
            const int q = i >> 1, ks = i & 1;
            if (i + 2 < 2 * P) a[i + 2] = a_read(i + 2);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float4 b = wr[q][nt][ks];
                acc[q][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b.x, acc[q][nt], 0, 0, 0);
                acc[q][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b.y, acc[q][nt], 0, 0, 0);
                acc[q][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, b.z, acc[q][nt], 0, 0, 0);
                acc[q][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, b.w, acc[q][nt], 0, 0, 0);
            }
            // this fragment's reload for the next slab goes straight behind the MFMAs that consumed it, 60 MFMAs ahead of its next
            // use, and stays there: left free, the scheduler sinks all sixteen reloads below the slab's last MFMAs and the next slab
            // waits for them at its first (profiles/r19_wino15_prefetch_isa.txt)
            w_issue(q, ks, nx);
            if (i + 2 < 2 * P) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 4 * NT, 0);
            __builtin_amdgcn_sched_group_barrier(0x020, NT, 0);
        }
    }
}

__device__ __forceinline__ float4 operator+(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 operator-(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

// The slab pipeline of F(2x2, 3x3): the MFMAs' A operands come straight from the halo.  Wave i owns row i of the 4x4 point grid,
// and row i of B^T d needs two rows of the tile's 4x4 window only: d0 - d2, d1 + d2, d2 - d1, d1 - d3.  Per 8-channel step a lane
// (tile lane & 31, channels 4 (lane >> 5) + 0..3, as the weights' k order requires) reads those two rows over the window's four
// columns, forms the row sum and from it the row's four points t0 - t2, t1 + t2, t2 - t1, t1 - t3 -- over the four waves the same
// additions, in the same order, as a transform of whole tiles would make, none of them twice.  No transformed tile in LDS; the
// halo is double-buffered instead (slab cb + 1 is stored while slab cb is multiplied), so a slab has one barrier.  The weights
// run one 8-channel step ahead in registers.  NORM: as HaloStage.
template <bool NORM>
__device__ __forceinline__ void wino3x3_slabs(const WinoK& p, const Patch& pt, float* Hs, int tid, int wave, f32x16 (&acc)[4][2]) {
    using HALO = Halo3x3;
    const int lane = tid & 63;
    HaloStage<HALO, NORM> hs(p, pt, tid);
    const WinoU u(p, lane);
    const int pt0 = 4 * wave, blk0 = 2 * pt.nb;
    float4 wr[4][2];
    wino_zero(acc);

    // rows ra, rb of the window and the sign of the second: t = d[ra] + sg * d[rb] (an fma by +-1 rounds as the sum itself)
    const int ra = wave == 0 ? 0 : wave == 2 ? 2 : 1, rb = wave == 2 ? 1 : wave == 3 ? 3 : 2;
    const float sg = wave == 1 ? 1.0f : -1.0f;
    const int tile = lane & 31;
    const int at0 = HALO::at(2 * (tile >> 3), 2 * (tile & 7)) + 4 * (lane >> 5);
    const int at_a = at0 + ra * HALO::lrow, at_b = at0 + rb * HALO::lrow;

    const int CB = p.cin / kWBK;
    // both first halos go out ahead of the first weights: at every arrival at the loop's store the halo is then older than the
    // eight fragments in flight, and the wait in front of it can leave those in flight (vmcnt retires in issue order)
    typename HaloStage<HALO, NORM>::Regs h0;
    hs.issue(0, h0);
    hs.issue(CB > 1 ? 1 : 0);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) wr[q][nt] = u.load(pt0 + q, blk0 + nt, 0);
    hs.store(Hs, h0);
    for (int cb = 0; cb < CB; ++cb) {
        const float* const H = Hs + (cb & 1) * HALO::floats;
        __syncthreads();   // slab cb is in H, and every wave has left the other buffer
        hs.store(Hs + (~cb & 1) * HALO::floats);
        // the last slabs re-issue the last one (and store it where nothing reads it): no branch, loads stay in bounds
        hs.issue(cb + 2 < CB ? cb + 2 : CB - 1);
        __builtin_amdgcn_sched_barrier(0);   // the loads go ahead of the products, as in wino_slabs_staged
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            float4 t[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float4 a = *reinterpret_cast<const float4*>(H + at_a + HALO::at(0, c) + 8 * ks);
                const float4 b = *reinterpret_cast<const float4*>(H + at_b + HALO::at(0, c) + 8 * ks);
                t[c] = make_float4(__builtin_fmaf(sg, b.x, a.x), __builtin_fmaf(sg, b.y, a.y), __builtin_fmaf(sg, b.z, a.z),
                                   __builtin_fmaf(sg, b.w, a.w));
            }
            const float4 v[4] = {t[0] - t[2], t[1] + t[2], t[2] - t[1], t[1] - t[3]};
            const int c8 = 2 * cb + ks + 1 < 2 * CB ? 2 * cb + ks + 1 : 2 * cb + ks;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    wino_mfma4(acc[q][nt], v[q], wr[q][nt]);
                    wr[q][nt] = u.load(pt0 + q, blk0 + nt, c8);   // the next step's fragment: 28 MFMAs hide the load
                    // ... and stays here: four MFMAs, then their fragment's reload.  Left free, the scheduler sinks the loads to
                    // their uses to save registers and every fragment is waited for within 3 MFMAs of its issue
                    // (profiles/r15_wino_prefetch_isa.txt)
                    __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
        }
    }
}

__device__ __forceinline__ float2 f2(float a, float b) { return make_float2(a, b); }
__device__ __forceinline__ float2 operator+(float2 a, float2 b) { return f2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 operator-(float2 a, float2 b) { return f2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 operator*(float s, float2 a) { return f2(s * a.x, s * a.y); }
__device__ __forceinline__ float2 fma2(float s, float2 a, float2 b) { return f2(__builtin_fmaf(s, a.x, b.x), __builtin_fmaf(s, a.y, b.y)); }

// F(4, 5): wave w = all 8 points x the w-th 32 of the workgroup's 128 outputs.  Input transform B^T d of one (tile, channel pair):
// 8 float2 taps at src -> the 8 points at dst; thread = (tile tid / 8, channel pair tid % 8).  VERT = false (1x5): tile t = (row
// t / 4, column group t % 4) reads halo pixels row * 20 + 4 (t % 4) + 0..7.  VERT = true (5x1): tile t = (row group t / 16, column
// t % 16) reads pixels (4 (t / 16) + 0..7) * 16 + t % 16.
template <bool VERT> struct Wino15 {
    using HALO = Halo15<VERT>;
    static constexpr int P = 8, NT = 1;
    __device__ static int pt0(int) { return 0; }
    __device__ static int blk0(int nb, int wave) { return 4 * nb + wave; }
    static constexpr int tap = (VERT ? HALO::W : 1) * HALO::ldh;   // floats between taps
    const float* src;
    float* dst;
    __device__ static int base(int t) { return VERT ? (4 * (t >> 4)) * HALO::W + (t & 15) : (t >> 2) * HALO::W + 4 * (t & 3); }
    // output pixel (dy, dx) in the patch of tile t, output i of the tile
    __device__ static int oy(int t, int i) { return VERT ? 4 * (t >> 4) + i : t >> 2; }
    __device__ static int ox(int t, int i) { return VERT ? (t & 15) : 4 * (t & 3) + i; }
    __device__ __forceinline__ Wino15(const float* Hs, float* Vs, int tid, int) {
        const int ttile = tid >> 3, tcp = tid & 7;
        src = Hs + base(ttile) * HALO::ldh + 2 * tcp;
        dst = Vs + ttile * kLDV + 2 * tcp;
    }
    __device__ __forceinline__ void operator()() const {
        float2 d[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = *reinterpret_cast<const float2*>(src + j * tap);
        // B^T d (rows 0 and 7 with the 21/4 pair, rows 1..6 as even / odd halves)
        float2 v[8];
        v[0] = (d[0] - d[6]) + 5.25f * (d[4] - d[2]);
        v[7] = (d[7] - d[1]) + 5.25f * (d[3] - d[5]);
        float2 te = (d[2] + d[6]) - 4.25f * d[4], to = (d[1] + d[5]) - 4.25f * d[3];
        v[1] = te + to;
        v[2] = te - to;
        te = (0.25f * d[2] + d[6]) - 1.25f * d[4];
        to = (0.5f * d[1] - 2.5f * d[3]) + 2.0f * d[5];
        v[3] = te + to;
        v[4] = te - to;
        te = (4.0f * d[2] + d[6]) - 5.0f * d[4];
        to = (2.0f * d[1] - 2.5f * d[3]) + 0.5f * d[5];
        v[5] = te + to;
        v[6] = te - to;
#pragma unroll
        for (int j = 0; j < 8; ++j) *reinterpret_cast<float2*>(dst + j * 32 * kLDV) = v[j];
    }
};

// ---- F(2x2, 3x3): 64 output channels per workgroup, wave w = points (w, 0..3) x both 32-channel halves
constexpr int kLDX = 32;                                    // output exchange: [wave][column fold][tile][32 channels]
constexpr int kXF = 4 * 2 * 32 * kLDX;                      // 8192 floats
constexpr int kSX = 2 * 4 * 32 * 2;                         // STATS: [32-channel half][wave][channel][sum, sum of squares]
// two halo buffers; after the last slab the exchange and the statistics reuse the space: 34 816 bytes, two workgroups per CU
constexpr int kSmem2 = 2 * Halo3x3::floats > kXF + kSX ? 2 * Halo3x3::floats : kXF + kSX;

// NORM: relu(norm(.)) on the operand (wino3x3_slabs).  RES: the residual merge relu(y + res) after the activation, as the direct
// kernel's plain epilogue.  STATS: per (patch, output channel) sum and sum of squares of the stored values, [B][tpi][Cout][2] for
// ofx_inorm_finalize_part, in a fixed order.  <false, false, false> is the update block's kernel.
template <bool NORM, bool RES, bool STATS>
__global__ __launch_bounds__(256, 2) void wino_conv_kernel(const WinoK p) {
    __shared__ __attribute__((aligned(16))) float smem[kSmem2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: the weight offsets stay scalar too
    const Patch pt = wino_patch(p);
    f32x16 acc[4][2];
    wino3x3_slabs<NORM>(p, pt, smem, tid, wave, acc);

    // ---- output transform and plain epilogue, one 32-channel half at a time through LDS
    const float act_lo = p.act == OFX_ACT_RELU ? 0.0f : -3.402823466e38f;   // OFX_ACT_NONE: a NaN sum becomes -FLT_MAX (see conv.hip)
    float* const X = smem;
    float* const Sx = smem + kXF;
    const int on = tid & 31, otx = tid >> 5;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        __syncthreads();   // nt 0: every wave's last operand reads are done; nt 1: the previous half has been read
        // column fold (A^T from the right) of this wave's row: t0 = M0 + M1 + M2, t1 = M1 - M2 - M3
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int tile = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
            const float m0 = acc[0][nt][e], m1 = acc[1][nt][e], m2 = acc[2][nt][e], m3 = acc[3][nt][e];
            X[((wave * 2 + 0) * 32 + tile) * kLDX + (lane & 31)] = m0 + m1 + m2;
            X[((wave * 2 + 1) * 32 + tile) * kLDX + (lane & 31)] = m1 - m2 - m3;
        }
        __syncthreads();
        const int oc = pt.nb * 64 + nt * 32 + on;
        if (oc < p.Cout) {   // (the same for lanes l and l ^ 32: the statistics' shuffle below stays within active lanes)
            const float sc = (p.scale ? p.scale[oc] : 1.0f) * p.alpha;
            const float sh = p.shift ? p.shift[oc] : 0.0f;
            float st_s = 0.0f, st_q = 0.0f;
#pragma unroll
            for (int ty = 0; ty < 4; ++ty) {
                const int tile = ty * 8 + otx;
                float x[4][2];
#pragma unroll
                for (int w = 0; w < 4; ++w)
#pragma unroll
                    for (int j = 0; j < 2; ++j) x[w][j] = X[((w * 2 + j) * 32 + tile) * kLDX + on];
                float r[2][2];
                if constexpr (RES) {
#pragma unroll
                    for (int a = 0; a < 2; ++a)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            r[a][j] = p.res[(((long)pt.pb * p.H + pt.y0 + 2 * ty + a) * p.W + pt.x0 + 2 * otx + j) * p.ldres + oc];
                }
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const float y = a == 0 ? x[0][j] + x[1][j] + x[2][j] : x[1][j] - x[2][j] - x[3][j];
                        const long pix = ((long)pt.pb * p.H + pt.y0 + 2 * ty + a) * p.W + pt.x0 + 2 * otx + j;
                        float v = fmaxf(y * sc + sh, act_lo);
                        if constexpr (RES) v = fmaxf(v + r[a][j], 0.0f);
                        p.out[pix * p.ldo + oc] = v;
                        if constexpr (STATS) {
                            st_s += v;
                            st_q = fmaf(v, v, st_q);
                        }
                    }
            }
            if constexpr (STATS) {   // the lane halves hold the patch's other tile column of the same channel
                st_s += __shfl_xor(st_s, 32, 64);
                st_q += __shfl_xor(st_q, 32, 64);
                if (lane < 32) {
                    Sx[((nt * 4 + wave) * 32 + on) * 2 + 0] = st_s;
                    Sx[((nt * 4 + wave) * 32 + on) * 2 + 1] = st_q;
                }
            }
        }
    }
    if constexpr (STATS) {   // the four waves' partials of each channel, added in wave order
        __syncthreads();
        const int nt = tid >> 5;
        const int oc = pt.nb * 64 + nt * 32 + on;
        if (tid < 64 && oc < p.Cout) {
            float s = 0.0f, q = 0.0f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                s += Sx[((nt * 4 + w) * 32 + on) * 2 + 0];
                q += Sx[((nt * 4 + w) * 32 + on) * 2 + 1];
            }
            const long row = (long)pt.pb * p.tpi + (pt.y0 >> 3) * p.tpr + (pt.x0 >> 4);
            p.stats[(row * p.Cout + oc) * 2 + 0] = s;
            p.stats[(row * p.Cout + oc) * 2 + 1] = q;
        }
    }
}

// ---- F(4, 5): 128 output channels per workgroup, wave w = all 8 points x 32 channels
template <bool VERT, int EPI>
__global__ __launch_bounds__(256, 2) void wino15_conv_kernel(const WinoK p) {
    using T = Wino15<VERT>;
    using HALO = typename T::HALO;
    __shared__ __attribute__((aligned(16))) float smem[HALO::floats + 8 * 32 * kLDV];   // halo + [point][tile][channel]: ~33 KB
    float* const Hs = smem;
    float* const Vs = smem + HALO::floats;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: the weight offsets stay scalar too
    const Patch pt = wino_patch(p);
    f32x16 acc[8][1];
    wino_slabs_staged<T>(p, pt, Hs, Vs, tid, wave, acc);

    // ---- output transform in registers, then the epilogue.  Element e of the C layout: tile (e & 3) + 8 (e >> 2) + 4 (lane >> 5),
    // output channel lane & 31 of the wave's 32.
    const int n = pt.nb * 128 + wave * 32 + (lane & 31);
    if (n >= p.Cout) return;   // no barrier follows
    const float sc = (p.scale ? p.scale[n] : 1.0f) * p.alpha;
    const float sh = p.shift ? p.shift[n] : 0.0f;
    const float act_lo = p.act == OFX_ACT_RELU ? 0.0f : -3.402823466e38f;   // OFX_ACT_NONE: a NaN sum becomes -FLT_MAX (see conv.hip)
    const int hd = p.Cout >> 1;
    const bool r_half = EPI == OFX_EPI_GRU_ZR && pt.nb * 128 >= hd;   // block-uniform (fits: hd % 128 == 0)
    // Four elements (16 outputs) per batch: every global read of the batch is issued before its arithmetic and stores (h is read
    // and written in place; interleaved, each read would wait behind the previous store).
#pragma unroll
    for (int eb = 0; eb < 16; eb += 4) {
        long pix[4][4];
        float y[4][4], ad[4][4], x1[4][4], x2[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = eb + u;
            const int tile = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
#pragma unroll
            for (int i = 0; i < 4; ++i) pix[u][i] = ((long)pt.pb * p.H + pt.y0 + T::oy(tile, i)) * p.W + pt.x0 + T::ox(tile, i);
            const float m0 = acc[0][0][e], m1 = acc[1][0][e], m2 = acc[2][0][e], m3 = acc[3][0][e];
            const float m4 = acc[4][0][e], m5 = acc[5][0][e], m6 = acc[6][0][e], m7 = acc[7][0][e];
            const float s12 = m1 + m2, d12 = m1 - m2, s34 = m3 + m4, d34 = m3 - m4, s56 = m5 + m6, d56 = m5 - m6;
            y[u][0] = m0 + s12 + s34 + s56;                          // A^T
            y[u][1] = d12 + 2.0f * d34 + 0.5f * d56;
            y[u][2] = s12 + 4.0f * s34 + 0.25f * s56;
            y[u][3] = d12 + 8.0f * d34 + 0.125f * d56 + m7;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ad[u][i] = p.addend ? p.addend[pix[u][i] * p.ldadd + n] : 0.0f;
                x1[u][i] = EPI == OFX_EPI_GRU_ZR ? (r_half ? p.aux_h[pix[u][i] * p.ldh + n - hd] : 1.0f)
                           : EPI == OFX_EPI_GRU_Q ? p.aux_z[pix[u][i] * p.Cout + n] : 0.0f;
                x2[u][i] = EPI == OFX_EPI_GRU_Q ? p.aux_h[pix[u][i] * p.ldh + n] : 0.0f;
            }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float v = y[u][i] * sc + sh + ad[u][i];
                if (EPI == OFX_EPI_PLAIN) {
                    p.out[pix[u][i] * p.ldo + n] = fmaxf(v, act_lo);
                } else if (EPI == OFX_EPI_GRU_ZR) {
                    const float g = ofx_sigmoid(v) * x1[u][i];            // z, or r * h
                    if (r_half) p.aux_rh[pix[u][i] * hd + n - hd] = g;
                    else p.aux_z[pix[u][i] * hd + n] = g;
                } else {
                    p.aux_h[pix[u][i] * p.ldh + n] = (1.0f - x1[u][i]) * x2[u][i] + x1[u][i] * ofx_tanh(v);
                }
            }
    }
}

// ---- F(4x4, 3x3): 36 point products per 16 outputs (2.25 multiplies per output), points {0, 1, -1, 2, -2, inf} (Lavin & Gray's
// matrices).  A workgroup of twelve waves owns a 16x32-pixel output patch -- 32 tiles of 4x4 -- and 64 output channels; wave
// (i, nt) owns row i of the 6x6 point grid and the nt-th 32 output channels: six accumulators.  The input transform B^T d B is
// split by what it costs.  Its row half -- row i of B^T d, a four-term combination of the window's rows per column and
// channel -- would be worked out by every row-wave and twice over the channel halves, each halo value read from LDS eight times:
// it is computed once per workgroup, a slab ahead, and staged in LDS as T (as F(4, 5) stages its transform).  Its column half --
// the six column points, twelve operations per channel -- is not redundant and stays in registers: a lane reads the six window
// columns of its wave's row of T and folds them into its A operands.  The halo (18 x 34 pixels) and T are staged per 8-channel
// slab, both double-buffered, one barrier per slab (the order of a trip: at the slab loop); a lane handles its four channels of
// the slab as two float2 halves (the register budget of three waves per SIMD, 168, does not hold the float4 form next to 96
// accumulators).  The weights run one slab ahead in registers, each fragment reloaded behind the MFMAs that consumed it.
//
// wino44_conv_kernel is the plain kernel (the update block's layers, the context encoder's conv1).  wino44_fused_kernel<NORM, RES,
// STATS> shares its body (conv_wino44_body.inl) and adds the encoders' options under the contracts of wino_conv_kernel.  NORM: the
// operand is relu((x - mean) * rstd) of image pt.pb (single segment), applied as the halo is stored, the padding that of the
// normalised map; the image's means and rstds are staged once in the LDS the slab staging leaves free (kNorm44 floats), since the
// registers of three waves per SIMD do not hold them across a slab.  RES: relu(y + res) after the activation.  STATS: per (16x32
// patch, output channel) the sum and the sum of squares of the stored values, [B][tpi][Cout][2], in a fixed order.
//
// Halo layout: a pixel's 8 channels are contiguous, the pixels (x, .. x + 3), x % 4 == 0, 32 contiguous floats, quads 34 floats
// apart, rows 308.  T keeps the layout of a halo row per (point row, tile row), 336 floats apart.  The operand ds_read_b64 of a
// half-wave (32 tiles: 8 along x, four pixels apart, 4 along y) then falls on 32 different bank pairs: 34 tx mod 64 = {0, 4, 8,
// 12, 34, 38, 42, 46}, 336 ty mod 64 = {0, 16, 32, 48} (tools/lds_bank_model.py --wino44).
struct Halo44 {
    static constexpr int W = 34, H = 18;
    static constexpr int lquad = 34, lrow = 308;
    static constexpr int floats = H * lrow;                 // 5544
    static constexpr int items = W * H * 2;                 // float4 pieces per slab: 1224
    static constexpr int threads = 768;
    static constexpr int slots = (items + threads - 1) / threads;   // 2
    __device__ __host__ static constexpr int at(int y, int x) { return y * lrow + (x >> 2) * lquad + (x & 3) * 8; }
    // The row-transformed slab T[point row i][tile row ty][x][8 channels]: row i of B^T d for the windows of tile row ty, pixels
    // laid out as in a halo row.  A (i, ty) row every 336 floats, 16 mod 64: the operand ds_read_b64 of a half-wave falls on 32
    // different bank pairs as before (34 tx mod 64 as above, 336 ty mod 64 = {0, 16, 32, 48}).
    static constexpr int ltrow = 336;
    static constexpr int tfloats = 6 * 4 * ltrow;           // 8064
    static constexpr int titems = 4 * W * 4;                // (tile row, x, channel pair): 544, one thread each
};
constexpr int kLDX4 = 40;                                   // output exchange: [wave][column fold b][16 tiles][32 channels at 40]
constexpr int kXF4 = 12 * 4 * 16 * kLDX4;                   // 30 720 floats: half the patch's tiles at a time
constexpr int kStage44 = 2 * (Halo44::floats + Halo44::tfloats);   // raw halo and T, both double-buffered: 27 216 floats
constexpr int kSmem44 = (kStage44 > kXF4 ? kStage44 : kXF4) * 4;   // bytes: 122 880, one workgroup per CU
// NORM: behind the staged slabs, per four channels [mean x 4 | rstd x 4]; most input channels that fit (a multiple of 16)
constexpr int kNorm44 = kSmem44 / 4 - kStage44;             // 3504 floats
constexpr int kNorm44MaxCin = kNorm44 / 2 / kWBK * kWBK;    // 1744
constexpr int kSX4 = 2 * 48 * 32 * 2;                       // STATS: [32-channel half][wave, lane / 8][channel][sum, sum of squares]
static_assert(kNorm44 >= 0 && kSX4 <= kXF4, "the fused options live in the plain kernel's LDS");

__global__ __launch_bounds__(768, 1) void wino44_conv_kernel(const WinoK p) {
    extern __shared__ __attribute__((aligned(16))) float smem44[];
    constexpr bool NORM = false, RES = false, STATS = false;
#include "conv_wino44_body.inl"
}

template <bool NORM, bool RES, bool STATS>
__global__ __launch_bounds__(768, 1) void wino44_fused_kernel(const WinoK p) {
    extern __shared__ __attribute__((aligned(16))) float smem44[];
#include "conv_wino44_body.inl"
}

// ---- host: one row per algorithm, the rule that picks a route for a descriptor, the launch

using WinoKernel = void (*)(WinoK);

// The kernels of an algorithm by launch variant.  3x3: NORM * 4 + RES * 2 + STATS (statistics are of raw outputs: never with a
// residual merge); F(4, 5): VERT * 3 + epilogue.
const WinoKernel kKernels22[8] = {wino_conv_kernel<false, false, false>, wino_conv_kernel<false, false, true>,
                                  wino_conv_kernel<false, true, false>,  nullptr,
                                  wino_conv_kernel<true, false, false>,  wino_conv_kernel<true, false, true>,
                                  wino_conv_kernel<true, true, false>,   nullptr};
const WinoKernel kKernels15[8] = {wino15_conv_kernel<true, OFX_EPI_PLAIN>,  wino15_conv_kernel<true, OFX_EPI_GRU_ZR>,
                                  wino15_conv_kernel<true, OFX_EPI_GRU_Q>,  wino15_conv_kernel<false, OFX_EPI_PLAIN>,
                                  wino15_conv_kernel<false, OFX_EPI_GRU_ZR>, wino15_conv_kernel<false, OFX_EPI_GRU_Q>,
                                  nullptr,                                  nullptr};
const WinoKernel kKernels44[8] = {wino44_conv_kernel,                       wino44_fused_kernel<false, false, true>,
                                  wino44_fused_kernel<false, true, false>,  nullptr,
                                  wino44_fused_kernel<true, false, false>,  wino44_fused_kernel<true, false, true>,
                                  wino44_fused_kernel<true, true, false>,   nullptr};

struct WinoAlg {
    bool one_d;                        // the layers it serves: 1x5 / 5x1, else 3x3
    int ph, pw;                        // output patch of a workgroup
    int points, outputs;               // point products and outputs per tile (the FLOPs it executes)
    int cblk;                          // output channels per workgroup
    int threads, dyn_lds;              // per workgroup; LDS bytes asked for at the launch (0: the kernel's own static arrays)
    const float* ofx_conv_desc::*u;    // its pre-transformed weights
    int tile;                          // the ofx_conv_desc.tile value that forces it
    long min_grid;                     // the grid gate: at least this many patches, or (per_block) patches x channel blocks,
    bool per_block;                    //   for the route to be taken unforced
    // What it admits besides the plain epilogue.  gates: an addend and the GRU gate epilogues, and none of the fused options; else
    // the fused options of the 3x3 kernels -- residual merge, relu(norm(.)) on the operand, epilogue statistics -- and no addend
    bool gates;
    bool norm_pair;                    // nmean and nrstd both or neither (else: a lone nrstd is ignored)
    int norm_max_cin;                  // most input channels under a fused norm
    int path, path_fused;              // ofx_conv_plan.path, without and with a fused option (statistics included)
    const WinoKernel* kernels;
};

// In the order of preference.  The grid gates:
//   F(4x4, 3x3) against F(2x2, 3x3): at least 768 workgroups, three for each of the chip's 256 CUs, where its workgroups run one
//     per CU.  Measured per layer shape at B = 4 ... 64 (profiles/r21_wino44_gate.txt): it wins at 768, 864,
//     1152, 1536, 2304 and 3072 workgroups and loses or ties at every measured grid of 576 or fewer.  Of the grids that end in a
//     nearly empty round only 864 was measured.  The encoders' stages with their fused variants
//     (profiles/r25_enc_wino44_gate.txt): wins at every grid from 768 on (x1.24 - x1.45), loses at 96 and wins by less at 192 and
//     384; the same gate.
//   F(2x2, 3x3) and F(4, 5) against the direct kernels and their small-grid schedules: 3x3, at least four workgroups per CU (two
//     rounds at its two per CU); 1x5 / 5x1, at least one 8x16 patch per CU (from six 512x768 pairs on; in isolation the kernel
//     already beat the direct one at four).
const WinoAlg kAlgs[] = {
    // F(4x4, 3x3); under a fused norm, as many input channels as the kernel stages means and rstds for
    {false, 16, 32, 36, 16, 64, 768, kSmem44, &ofx_conv_desc::wino4_w, OFX_CONV_TILE_WINOGRAD4, 768, true,
     false, true, kNorm44MaxCin, kPathWino44, kPathWino44Fused, kKernels44},
    // F(2x2, 3x3)
    {false, 8, 16, 16, 4, 64, 256, 0, &ofx_conv_desc::wino_w, OFX_CONV_TILE_WINOGRAD, 1024, true,
     false, false, 0x7FFFFFFF, kPathWino3x3, kPathWino3x3, kKernels22},
    // F(4, 5)
    {true, 8, 16, 8, 4, 128, 256, 0, &ofx_conv_desc::wino_w, OFX_CONV_TILE_WINOGRAD, 256, false,
     true, false, 0, kPathWino15, kPathWino15, kKernels15},
};
constexpr int kNumAlgs = sizeof kAlgs / sizeof kAlgs[0];

bool is_1d(int KH, int KW) { return (KH == 1 && KW == 5) || (KH == 5 && KW == 1); }

// Shape test of row `a`: fp32, one problem, stride 1, 3x3 (pad 1, 1), 1x5 (pad 0, 2) or 5x1 (pad 2, 0) keeping the map size, a map
// of whole patches, 16-channel slabs that never straddle the two input segments, the row's operand set and aligned.  Epilogues:
// plain (ReLU or identity, scale / shift, strided destination); the 3x3 rows without addend, optionally with the residual merge
// relu(y + res) and / or relu(norm(.)) fused into the operand (single segment, aligned mean / rstd: the encoders' layers); F(4, 5)
// with no fused norm or residual, plain (optional addend) or a GRU gate epilogue whose z | r split falls on a 128-channel block
// boundary.
bool wino_fits(const WinoAlg& a, const ofx_conv_desc* d) {
    const int cin = d->c0 + d->c1;
    const float* const u = d->*a.u;
    const bool plain = d->epi == OFX_EPI_PLAIN && d->out != nullptr && d->ldo >= d->Cout && (d->act == OFX_ACT_NONE || d->act == OFX_ACT_RELU);
    const bool shape = a.one_d ? is_1d(d->KH, d->KW) : d->KH == 3 && d->KW == 3;
    bool epi;
    if (a.gates) {
        epi = !d->nmean && !d->res && (plain || (d->epi == OFX_EPI_GRU_ZR && (d->Cout / 2) % a.cblk == 0) || d->epi == OFX_EPI_GRU_Q);
    } else {
        epi = plain && !d->addend && (!d->res || d->ldres >= d->Cout) && (!a.norm_pair || (d->nmean != nullptr) == (d->nrstd != nullptr)) &&
              (!d->nmean || (d->nrstd && !d->in1 && d->c0 <= a.norm_max_cin && ofx_aligned16(d->nmean) && ofx_aligned16(d->nrstd)));
    }
    return shape && epi && d->padH == d->KH / 2 && d->padW == d->KW / 2 && d->precision == OFX_PREC_FP32 && d->nz <= 1 && d->stride == 1 &&
           d->Hout == d->Hin && d->Wout == d->Win && d->Hin % a.ph == 0 && d->Win % a.pw == 0 && cin % kWBK == 0 && d->c0 % kWBK == 0 &&
           u != nullptr && ofx_aligned16(u);
}

// Rows per image of the instance-norm partial sums row `a` leaves for a fitting `d` (one per patch), or 0 when it cannot produce
// them: the 3x3 rows, raw outputs only (identity, no residual), as the direct kernel's epilogue statistics.
int wino_stats_rows(const WinoAlg& a, const ofx_conv_desc* d) {
    return !a.gates && d->act == OFX_ACT_NONE && !d->res ? (d->Hin / a.ph) * (d->Win / a.pw) : 0;
}

// The argument block of a fitting descriptor.  Byte extents and the grid stay below 2^31 (32-bit offsets through buffer
// descriptors); the 3x3 rows also ask that of the destination's float count, the F(4, 5) row does not.
int wino_args(const WinoAlg& a, const ofx_conv_desc* d, float alpha, float* stats, WinoK* out) {
    WinoK k{};
    k.in0 = d->in0; k.in1 = d->in1; k.u = d->*a.u; k.scale = d->scale; k.shift = d->shift; k.addend = d->addend; k.out = d->out;
    k.res = d->res; k.nmean = d->nmean; k.nrstd = d->nrstd; k.stats = stats;
    k.aux_z = d->aux_z; k.aux_rh = d->aux_rh; k.aux_h = d->aux_h;
    k.ld0 = d->ld0; k.c0 = d->c0; k.ld1 = d->ld1; k.cin = d->c0 + d->c1; k.ldo = d->ldo; k.ldadd = d->ldadd; k.ldh = d->ldh;
    k.ldres = d->ldres;
    k.H = d->Hin; k.W = d->Win; k.Cout = d->Cout; k.act = d->act;
    k.nblk = (d->Cout + a.cblk - 1) / a.cblk;
    k.nb32 = a.cblk / 32 * k.nblk;
    k.tpr = d->Win / a.pw;
    k.tpi = (d->Hin / a.ph) * k.tpr;
    const long mtiles = (long)d->B * k.tpi;
    const long npix = (long)d->B * d->Hin * d->Win;
    const long ext0 = ((npix - 1) * d->ld0 + d->c0) * 4, ext1 = d->in1 ? ((npix - 1) * d->ld1 + d->c1) * 4 : 0;
    const long extu = (long)a.points * k.nb32 * 32 * k.cin * 4;
    OFX_REQUIRE(ext0 < (1L << 31) - 64 && ext1 < (1L << 31) - 64 && extu < (1L << 31) - 64, OFX_EINVAL);
    OFX_REQUIRE(mtiles * k.nblk < (1L << 31) && (a.one_d || npix * d->ldo < (1L << 31)), OFX_EINVAL);
    k.mtiles = (int)mtiles;
    k.bytes0 = (int)ext0; k.bytes1 = (int)ext1; k.bytesu = (int)extu;
    k.alpha = alpha;
    // whole channel quads of the 3x3 epilogue may move as 16 bytes (decided here, once per launch; else 4 bytes at a time)
    k.vec4 = ofx_aligned16(d->out) && d->ldo % 4 == 0 && ofx_aligned16(d->scale) && ofx_aligned16(d->shift) &&
             (!d->res || (ofx_aligned16(d->res) && d->ldres % 4 == 0));
    *out = k;
    return 0;
}

// Launch variant `v` of row `a`, the stop event (may be null) riding on the kernel (OFX_LAUNCH).  More than 64 KB of LDS is allowed
// once per kernel and device (as corr_split.hip).
int wino_launch_kernel(const WinoAlg& a, int v, const WinoK& k, hipStream_t s, hipEvent_t stop_event) {
    const WinoKernel kernel = v >= 0 && v < 8 ? a.kernels[v] : nullptr;
    OFX_REQUIRE(kernel != nullptr, OFX_EINVAL);
    if (a.dyn_lds > 65536) {
        static bool allowed[64][kNumAlgs][8] = {};
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return OFX_EINVAL;
        bool& ok = allowed[dev][&a - kAlgs][v];
        if (!ok) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, a.dyn_lds);
            if (e != hipSuccess) return (int)e;
            ok = true;
        }
    }
    const dim3 grid((unsigned)(k.mtiles * k.nblk), 1, 1), block(a.threads, 1, 1);
    if (stop_event) hipExtLaunchKernelGGL(kernel, grid, block, a.dyn_lds, s, nullptr, stop_event, 0, k);
    else hipLaunchKernelGGL(kernel, grid, block, a.dyn_lds, s, k);
    return ofx_launch_status();
}

}  // namespace

// Which Winograd route, if any, takes a validated descriptor: pure (no HIP call, no environment, no global state).  The rows are
// tried in their order of preference.  A row is a candidate when its tile value forces it, or under the launcher's own rule
// (tile = 0) when its switch is not off and its operand is set; it takes the layer when the layer fits it (wino_fits, no pooled
// volume, and for requested statistics a row that leaves them and room for them) and, unforced, its grid gate holds.  Any other
// layer goes on to the direct kernels (path 0) -- F(4, 5) never produces statistics, so a request for them does -- except under a
// forced tile, which runs its route or is rejected.
int ofx_conv_wino_choose(const ofx_conv_desc* d, bool want_stats, size_t stats_cap, bool pool, bool no_wino, bool no_wino15, bool no_wino44,
                         OfxWinoChoice* c) {
    *c = OfxWinoChoice{};
    const bool off[kNumAlgs] = {no_wino44, no_wino, no_wino15};   // (in the order of kAlgs)
    const bool one_d = is_1d(d->KH, d->KW);
    for (int i = 0; i < kNumAlgs; ++i) {
        const WinoAlg& a = kAlgs[i];
        const bool force = d->tile == a.tile;
        if (a.one_d != one_d || !(force || (d->tile == 0 && !off[i] && d->*a.u))) continue;
        const int srows = want_stats ? wino_stats_rows(a, d) : 0;
        const bool stats_ok = !want_stats || (srows > 0 && (size_t)d->B * srows * d->Cout * 2 <= stats_cap);
        if (!(stats_ok && !pool && wino_fits(a, d))) continue;
        const long patches = (long)d->B * (d->Hin / a.ph) * (d->Win / a.pw);
        if (!force && patches * (a.per_block ? (d->Cout + a.cblk - 1) / a.cblk : 1) < a.min_grid) continue;
        c->path = want_stats || d->res || d->nmean || d->nrstd ? a.path_fused : a.path;
        c->stats_rows = srows;
        // multiplies x 2: `points` point products per tile of `outputs` outputs, input channel and output channel
        c->flops = 2.0 * a.points * ((double)d->B * d->Hout * d->Wout / a.outputs) * (double)(d->c0 + d->c1) * d->Cout;
        return 0;
    }
    return d->tile == OFX_CONV_TILE_WINOGRAD || d->tile == OFX_CONV_TILE_WINOGRAD4 ? OFX_EINVAL : 0;
}

// The launch of the route ofx_conv_wino_choose gave for `d` (path != 0).  stats: null, or the room the choice was made with, for
// its stats_rows > 0 rows per image.
int ofx_conv_wino_launch(const ofx_conv_desc* d, int path, float alpha, float* stats, hipStream_t s, hipEvent_t stop_event) {
    const WinoAlg* a = nullptr;
    for (const WinoAlg& row : kAlgs)
        if (path == row.path || path == row.path_fused) a = &row;
    OFX_REQUIRE(a && (!stats || wino_stats_rows(*a, d) > 0), OFX_EINVAL);
    WinoK k;
    if (int st = wino_args(*a, d, alpha, stats, &k)) return st;
    const int v = a->gates ? (d->epi >= OFX_EPI_PLAIN && d->epi <= OFX_EPI_GRU_Q ? (d->KH == 5 ? 0 : 3) + d->epi : -1)
                           : (k.nmean ? 4 : 0) | (k.res ? 2 : 0) | (k.stats ? 1 : 0);
    return wino_launch_kernel(*a, v, k, s, stop_event);
}

namespace {

// Host: U = T g per (output, input) channel pair of OIHW weights w (`taps` contiguous floats per pair) in float64 (`xf` writes the
// `points` values), rounded once to fp32, in the fused kernel's operand order: [points][Cout rounded up to `cblk`, as 32-channel
// blocks][Cin / 8][2][32][4], i.e. point q, output channel o = 32 nb + n, input channel c = 8 c8 + 4 h + e at float
// (((q * NB + nb) * Cin / 8 + c8) * 2 + h) * 128 + 4 n + e.  Padded output channels are zero.  Returns the float count (out may be
// NULL to query it) or OFX_EINVAL.
template <class XF>
long wino_weight(const float* w, int Cout, int Cin, int taps, int points, int cblk, float* out, XF xf) {
    OFX_REQUIRE(Cout > 0 && Cin > 0 && Cin % kWBK == 0, OFX_EINVAL);
    const int nb32 = cblk / 32 * ((Cout + cblk - 1) / cblk);
    const long n = (long)points * nb32 * 32 * Cin;
    if (!out) return n;
    OFX_REQUIRE(w != nullptr, OFX_EINVAL);
    std::memset(out, 0, (size_t)n * sizeof(float));
    double u[16];
    for (int o = 0; o < Cout; ++o)
        for (int c = 0; c < Cin; ++c) {
            xf(w + ((size_t)o * Cin + c) * taps, u);
            for (int q = 0; q < points; ++q) {
                const long at = ((((long)q * nb32 + o / 32) * (Cin / 8) + c / 8) * 2 + (c % 8) / 4) * 128 + 4 * (o % 32) + c % 4;
                out[at] = (float)u[q];
            }
        }
    return n;
}

}  // namespace

// 3x3: U = G g G^T, point (i, j) = 4 i + j; Cout rounded up to 64.
extern "C" long ofx_wino_conv_weight(const float* w, int Cout, int Cin, float* out) {
    return wino_weight(w, Cout, Cin, 9, 16, 64, out, [](const float* g, double* u) {
        static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
        double gg[4][3];   // G g
        for (int i = 0; i < 4; ++i)
            for (int x = 0; x < 3; ++x) gg[i][x] = G[i][0] * g[x] + G[i][1] * g[3 + x] + G[i][2] * g[6 + x];
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) u[4 * i + j] = gg[i][0] * G[j][0] + gg[i][1] * G[j][1] + gg[i][2] * G[j][2];
    });
}

// 1x5 or 5x1 (the 5 taps are contiguous in either orientation): U = G g; Cout rounded up to 128.  G rows: the points 0, 1, -1, 2,
// -2, 1/2, -1/2 scaled by 1 / prod_{k != j} (a_j - a_k) (row 0 sign-flipped, with B^T's), and inf.
extern "C" long ofx_wino15_conv_weight(const float* w, int Cout, int Cin, int KH, int KW, float* out) {
    OFX_REQUIRE(is_1d(KH, KW), OFX_EINVAL);
    return wino_weight(w, Cout, Cin, 5, 8, 128, out, [](const float* g, double* u) {
        static const double G[8][5] = {
            {1, 0, 0, 0, 0},
            {-2.0 / 9, -2.0 / 9, -2.0 / 9, -2.0 / 9, -2.0 / 9},
            {-2.0 / 9, 2.0 / 9, -2.0 / 9, 2.0 / 9, -2.0 / 9},
            {1.0 / 90, 1.0 / 45, 2.0 / 45, 4.0 / 45, 8.0 / 45},
            {1.0 / 90, -1.0 / 45, 2.0 / 45, -4.0 / 45, 8.0 / 45},
            {32.0 / 45, 16.0 / 45, 8.0 / 45, 4.0 / 45, 2.0 / 45},
            {32.0 / 45, -16.0 / 45, 8.0 / 45, -4.0 / 45, 2.0 / 45},
            {0, 0, 0, 0, 1},
        };
        for (int q = 0; q < 8; ++q) {
            u[q] = 0.0;
            for (int t = 0; t < 5; ++t) u[q] += G[q][t] * (double)g[t];
        }
    });
}

// 3x3, F(4x4): U = G g G^T over the points {0, 1, -1, 2, -2, inf}, point (i, j) = 6 i + j, in float64, rounded once; Cout rounded
// up to 64 (NB = 2 * ceil(Cout / 64) blocks of 32, padded output channels zero).  The kernel's operand order, 512-byte fragments
// of one point, 32 outputs and a half step of four channels: [36][NB][Cin / 8][2][2][32][2], i.e. point q, output channel
// o = 32 nb + n, input channel c = 8 c8 + 4 h + 2 s + e at float ((((q * NB + nb) * Cin / 8 + c8) * 2 + s) * 2 + h) * 64 + 2 n + e.
extern "C" long ofx_wino44_conv_weight(const float* w, int Cout, int Cin, float* out) {
    OFX_REQUIRE(Cout > 0 && Cin > 0 && Cin % kWBK == 0, OFX_EINVAL);
    const int nb32 = 2 * ((Cout + 63) / 64);
    const long n = 36L * nb32 * 32 * Cin;
    if (!out) return n;
    OFX_REQUIRE(w != nullptr, OFX_EINVAL);
    std::memset(out, 0, (size_t)n * sizeof(float));
    static const double G[6][3] = {{1.0 / 4, 0, 0},           {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                   {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
    for (int o = 0; o < Cout; ++o)
        for (int c = 0; c < Cin; ++c) {
            const float* g = w + ((size_t)o * Cin + c) * 9;
            double gg[6][3];   // G g
            for (int i = 0; i < 6; ++i)
                for (int x = 0; x < 3; ++x) gg[i][x] = G[i][0] * g[x] + G[i][1] * g[3 + x] + G[i][2] * g[6 + x];
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 6; ++j) {
                    const double u = gg[i][0] * G[j][0] + gg[i][1] * G[j][1] + gg[i][2] * G[j][2];
                    const long q = 6 * i + j;
                    const long at = ((((q * nb32 + o / 32) * (Cin / 8) + c / 8) * 2 + (c % 4) / 2) * 2 + (c % 8) / 4) * 64 + 2 * (o % 32) + c % 2;
                    out[at] = (float)u;
                }
        }
    return n;
}
