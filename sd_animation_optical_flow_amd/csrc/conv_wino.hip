// Fused Winograd F(2x2, 3x3) convolution on the fp32 matrix cores of gfx950.
//
// For the stride-1 3x3 "same" layers of the update block (convc2, conv, flow_head.conv1, convf2 at 1/8 resolution) the direct
// halo-patch kernel of conv.hip runs at ~0.9 of the fp32 MFMA peak, so the only way to take real time off them is to execute fewer
// multiplies.  F(2x2, 3x3) produces a 2x2 output tile from a 4x4 input tile with 16 point-wise products per (input, output)
// channel pair instead of 36: 4 multiplies per output pixel instead of 9.
//
//   Y = A^T [ (G g G^T) (.) (B^T d B) ] A     (Lavin & Gray, "Fast Algorithms for Convolutional Neural Networks", 2016)
//
// Everything between the input and the output stays on chip -- the unfused form (transformed input and output through HBM) costs as
// much traffic as it saves multiplies ("Winograd"):
//   * a workgroup owns one 8x16-pixel output patch (32 Winograd tiles of 2x2) and 64 output channels;
//   * per 16-channel slab the 10x18 input halo is staged in LDS once (buffer descriptors return the zero padding), every thread
//     applies B^T d B to one (tile, channel pair) -- additions only -- and writes the 16 transformed values to LDS;
//   * wave w owns the four points (w, 0..3) of the 4x4 transform grid: for each it runs the point-wise GEMM
//     [32 tiles x 16 channels] x [16 channels x 64 outputs] on v_mfma_f32_32x32x2_f32 into 2 x 16 accumulators;
//   * the pre-transformed weights U = G g G^T (host, float64, one rounding: ofx_wino_conv_weight) are stored in the MFMA's B-operand
//     lane order, so every wave loads its own 1 KB fragments straight into registers, one slab ahead, with fully contiguous loads;
//   * after the last slab, each wave folds its four points along the transform's column (A^T from the right), the partial rows
//     meet in LDS, and the row fold (A^T from the left) feeds the plain epilogue: scale / shift, ReLU, strided store.
// Executed multiplies per output: 16 / 4 = 4 per (cin, cout) against 9 for the direct kernel.
#include "ofx_internal.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

namespace {

constexpr int kWBK = 16;                    // channels per slab
constexpr int kHaloW = 18, kHaloH = 10;     // input halo of an 8x16 output patch
constexpr int kHaloPix = kHaloW * kHaloH;   // 180
constexpr int kHaloItems = kHaloPix * (kWBK / 4);   // float4 pieces per slab: 720
constexpr int kHaloSlots = (kHaloItems + 255) / 256;   // per thread: 3
// halo pixel stride 24 floats: the transform's float2 reads (four tiles two pixels apart per half-wave) land in disjoint banks
constexpr int kLDH = 24;
// transformed tile row stride 20 floats: conflict-free ds_read_b128 A fragments (as the direct kernel's LDK)
constexpr int kLDV = kWBK + 4;
constexpr int kLDX = 32;                    // output exchange: [wave][column fold][tile][32 channels]
constexpr int kHaloF = kHaloPix * kLDH;     // 4320 floats
constexpr int kVF = 16 * 32 * kLDV;         // 10240 floats
constexpr int kXF = 4 * 2 * 32 * kLDX;      // 8192 floats (reuses the halo / V space after the last slab)
constexpr int kSmemF = kHaloF + kVF;        // 58 240 bytes: two workgroups per CU
static_assert(kXF <= kSmemF, "exchange must fit");
constexpr int kOOB = 0x7FFFFFF0;

struct WinoK {
    const float* in0;
    const float* in1;
    const float* u;          // ofx_wino_conv_weight layout
    const float* scale;
    const float* shift;
    float* out;
    int ld0, c0, ld1, cin, ldo;
    int H, W, Cout, act;
    int nblk;                // 64-channel output blocks
    int nb32;                // 32-channel blocks of u
    int tpr, tpi, mtiles;    // patches per image row / per image, patches in all
    int bytes0, bytes1, bytesu;
    float alpha;
};

__device__ __forceinline__ float2 f2sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 f2add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }

__global__ __launch_bounds__(256, 2) void wino_conv_kernel(const WinoK p) {
    typedef int v4i __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) float smem[kSmemF];
    float* const Hs = smem;
    float* const Vs = smem + kHaloF;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: the weight offsets below stay scalar too

    // the XCD remap of conv.hip: the output blocks of one patch run back to back on one XCD (shared halo in its L2)
    const int nblk = p.mtiles * p.nblk;
    const int bid = blockIdx.x;
    const int q8 = nblk >> 3, r8 = nblk & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int L = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
    const int nb = L % p.nblk, mt = L / p.nblk;
    const int pb = mt / p.tpi;
    const int trem = mt - pb * p.tpi;
    const int py = trem / p.tpr;
    const int y0 = py * 8, x0 = (trem - py * p.tpr) * 16;

    // ---- halo staging: item i = (pixel i / 4, float4 slot i % 4) of the slab, pixels row-major over the 10 x 18 halo
    const float* in1s = p.in1 ? p.in1 : p.in0;
    const int bytes1s = p.in1 ? p.bytes1 : p.bytes0;
    int hpix[kHaloSlots];
    unsigned hok = 0;
#pragma unroll
    for (int k = 0; k < kHaloSlots; ++k) {
        const int i = tid + 256 * k;
        const int pix = i >> 2;
        const int hy = pix / kHaloW, hx = pix - hy * kHaloW;
        const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
        const bool ok = i < kHaloItems && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
        hpix[k] = ok ? (pb * p.H + gy) * p.W + gx : 0;
        hok |= (ok ? 1u : 0u) << k;
    }
    const int hq = (tid & 3) * 16;   // byte offset of this thread's float4 slot (256 % 4 == 0: the same for every k)
    float4 pa[kHaloSlots];
    auto a_issue = [&](int cb) __attribute__((always_inline)) {
        const int c = cb * kWBK;
        const bool s0 = c < p.c0;    // wave-uniform
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(s0 ? p.in0 : in1s), (short)0, s0 ? p.bytes0 : bytes1s, 0x00020000);
        const int so = (s0 ? c : c - p.c0) * 4;
        const int ldb = (s0 ? p.ld0 : p.ld1) * 4;
#pragma unroll
        for (int k = 0; k < kHaloSlots; ++k) {
            const int vo = ((hok >> k) & 1u) ? hpix[k] * ldb + hq : kOOB;
            v4i t = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, so, 0);
            pa[k] = *reinterpret_cast<float4*>(&t);
        }
    };

    // ---- weights: wave w, point (w, q), 32-channel block 2 nb + nt, 8-channel chunk 2 cb + ks -> one contiguous 1 KB fragment
    const __amdgpu_buffer_rsrc_t rsu = __builtin_amdgcn_make_buffer_rsrc((void*)p.u, (short)0, p.bytesu, 0x00020000);
    const int c8n = p.cin >> 3;
    const int wlane = lane * 16;
    float4 wr[4][2][2];
    auto w_issue = [&](int q, int cb) __attribute__((always_inline)) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int so = (((wave * 4 + q) * p.nb32 + 2 * nb + nt) * c8n + 2 * cb + ks) * 1024;   // scalar
                v4i t = __builtin_amdgcn_raw_buffer_load_b128(rsu, wlane, so, 0);
                wr[q][nt][ks] = *reinterpret_cast<float4*>(&t);
            }
    };

    f32x16 acc[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[q][nt][e] = 0.f;

    // input transform: thread = (tile row = wave, tile column tx, channel pair cp)
    const int ttx = lane >> 3, tcp = lane & 7;
    const int ttile = wave * 8 + ttx;
    const float* const tsrc = Hs + (2 * wave * kHaloW + 2 * ttx) * kLDH + 2 * tcp;
    float* const tdst = Vs + ttile * kLDV + 2 * tcp;
    // A fragment: tile = lane & 31, channels 8 ks + 4 (lane >> 5) + 0..3 (the k order the weights are stored in)
    const float* const afrag = Vs + (wave * 4 * 32 + (lane & 31)) * kLDV + 4 * (lane >> 5);

    const int CB = p.cin / kWBK;
    a_issue(0);
#pragma unroll
    for (int q = 0; q < 4; ++q) w_issue(q, 0);
    for (int cb = 0; cb < CB; ++cb) {
        const int nx = cb + 1 < CB ? cb + 1 : cb;   // the last slab re-issues itself: no branch, loads stay in bounds
#pragma unroll
        for (int k = 0; k < kHaloSlots; ++k) {
            const int i = tid + 256 * k;
            if (kHaloSlots * 256 > kHaloItems && k == kHaloSlots - 1 && i >= kHaloItems) break;
            *reinterpret_cast<float4*>(&Hs[(i >> 2) * kLDH + (i & 3) * 4]) = pa[k];
        }
        __syncthreads();
        {
            float2 d[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) d[r][c] = *reinterpret_cast<const float2*>(tsrc + (r * kHaloW + c) * kLDH);
            float2 t[4][4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {           // B^T d
                t[0][c] = f2sub(d[0][c], d[2][c]);
                t[1][c] = f2add(d[1][c], d[2][c]);
                t[2][c] = f2sub(d[2][c], d[1][c]);
                t[3][c] = f2sub(d[1][c], d[3][c]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {           // (B^T d) B
                float2 v[4];
                v[0] = f2sub(t[i][0], t[i][2]);
                v[1] = f2add(t[i][1], t[i][2]);
                v[2] = f2sub(t[i][2], t[i][1]);
                v[3] = f2sub(t[i][1], t[i][3]);
#pragma unroll
                for (int j = 0; j < 4; ++j) *reinterpret_cast<float2*>(tdst + (i * 4 + j) * 32 * kLDV) = v[j];
            }
        }
        __syncthreads();
        a_issue(nx);   // the next slab's halo lands during this slab's products (issued here, not live across the transform)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const float4 a = *reinterpret_cast<const float4*>(afrag + q * 32 * kLDV + 8 * ks);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const float4 b = wr[q][nt][ks];
                    acc[q][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc[q][nt], 0, 0, 0);
                    acc[q][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc[q][nt], 0, 0, 0);
                    acc[q][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc[q][nt], 0, 0, 0);
                    acc[q][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc[q][nt], 0, 0, 0);
                }
            }
            w_issue(q, nx);   // this point's fragments for the next slab: the rest of the slab hides the load
        }
    }

    // ---- output transform and plain epilogue, one 32-channel half at a time through LDS
    const float act_lo = p.act == OFX_ACT_RELU ? 0.0f : -3.402823466e38f;
    float* const X = smem;
    const int on = tid & 31, otx = tid >> 5;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        __syncthreads();   // nt 0: every wave's last fragment reads are done; nt 1: the previous half has been read
        // column fold (A^T from the right) of this wave's row: t0 = M0 + M1 + M2, t1 = M1 - M2 - M3
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int tile = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
            const float m0 = acc[0][nt][e], m1 = acc[1][nt][e], m2 = acc[2][nt][e], m3 = acc[3][nt][e];
            X[((wave * 2 + 0) * 32 + tile) * kLDX + (lane & 31)] = m0 + m1 + m2;
            X[((wave * 2 + 1) * 32 + tile) * kLDX + (lane & 31)] = m1 - m2 - m3;
        }
        __syncthreads();
        const int oc = nb * 64 + nt * 32 + on;
        if (oc < p.Cout) {
            const float sc = (p.scale ? p.scale[oc] : 1.0f) * p.alpha;
            const float sh = p.shift ? p.shift[oc] : 0.0f;
#pragma unroll
            for (int ty = 0; ty < 4; ++ty) {
                const int tile = ty * 8 + otx;
                float x[4][2];
#pragma unroll
                for (int w = 0; w < 4; ++w)
#pragma unroll
                    for (int j = 0; j < 2; ++j) x[w][j] = X[((w * 2 + j) * 32 + tile) * kLDX + on];
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const float y = a == 0 ? x[0][j] + x[1][j] + x[2][j] : x[1][j] - x[2][j] - x[3][j];
                        const long pix = ((long)pb * p.H + y0 + 2 * ty + a) * p.W + x0 + 2 * otx + j;
                        p.out[pix * p.ldo + oc] = fmaxf(y * sc + sh, act_lo);
                    }
            }
        }
    }
}

}  // namespace

// Shape test for the fused kernel: fp32, one problem, 3x3 stride 1 'same', a map of whole 8x16 patches, 16-channel slabs that never
// straddle the two input segments, the plain epilogue without fused norm, residual or addend, ReLU or identity.
bool ofx_conv_wino_fits(const ofx_conv_desc* d) {
    const int cin = d->c0 + d->c1;
    return d->precision == OFX_PREC_FP32 && (d->nz <= 1) && d->KH == 3 && d->KW == 3 && d->stride == 1 && d->padH == 1 &&
           d->padW == 1 && d->Hout == d->Hin && d->Wout == d->Win && d->Hin % 8 == 0 && d->Win % 16 == 0 && cin % kWBK == 0 &&
           d->c0 % kWBK == 0 && d->epi == OFX_EPI_PLAIN && !d->nmean && !d->res && !d->addend && d->out != nullptr &&
           d->ldo >= d->Cout && (d->act == OFX_ACT_NONE || d->act == OFX_ACT_RELU) && d->wino_w != nullptr && ofx_aligned16(d->wino_w);
}

long ofx_conv_wino_blocks(const ofx_conv_desc* d) {
    return (long)d->B * (d->Hin / 8) * (d->Win / 16) * ((d->Cout + 63) / 64);
}

// Multiplies the fused kernel executes for `d` (x 2 FLOPs): 16 point products per 2x2 tile, input channel and output channel
double ofx_conv_wino_flops(const ofx_conv_desc* d) {
    return 2.0 * 16.0 * ((double)d->B * d->Hout * d->Wout / 4.0) * (double)(d->c0 + d->c1) * d->Cout;
}

// The caller has validated the descriptor (ofx_conv2d_alpha) and ofx_conv_wino_fits(d).
int ofx_conv_wino_launch(const ofx_conv_desc* d, float alpha, hipStream_t s) {
    WinoK k;
    k.in0 = d->in0; k.in1 = d->in1; k.u = d->wino_w; k.scale = d->scale; k.shift = d->shift; k.out = d->out;
    k.ld0 = d->ld0; k.c0 = d->c0; k.ld1 = d->ld1; k.cin = d->c0 + d->c1; k.ldo = d->ldo;
    k.H = d->Hin; k.W = d->Win; k.Cout = d->Cout; k.act = d->act;
    k.nblk = (d->Cout + 63) / 64;
    k.nb32 = 2 * k.nblk;
    k.tpr = d->Win / 16;
    k.tpi = (d->Hin / 8) * k.tpr;
    const long mtiles = (long)d->B * k.tpi;
    const long npix = (long)d->B * d->Hin * d->Win;
    const long ext0 = ((npix - 1) * d->ld0 + d->c0) * 4, ext1 = d->in1 ? ((npix - 1) * d->ld1 + d->c1) * 4 : 0;
    const long extu = 16L * k.nb32 * 32 * k.cin * 4;
    OFX_REQUIRE(ext0 < (1L << 31) - 64 && ext1 < (1L << 31) - 64 && extu < (1L << 31) - 64, OFX_EINVAL);
    OFX_REQUIRE(mtiles * k.nblk < (1L << 31) && npix * d->ldo < (1L << 31), OFX_EINVAL);
    k.mtiles = (int)mtiles;
    k.bytes0 = (int)ext0; k.bytes1 = (int)ext1; k.bytesu = (int)extu;
    k.alpha = alpha;
    dim3 grid((unsigned)(k.mtiles * k.nblk), 1, 1), block(256, 1, 1);
    OFX_LAUNCH(wino_conv_kernel, grid, block, s, k);
    return ofx_launch_status();
}

// Host: OIHW 3x3 weights -> U = G g G^T per (output, input) channel pair in float64, rounded once to fp32, in the fused kernel's
// operand order: [16 points][Cout rounded up to 64, as 32-channel blocks][Cin / 8][2][32][4], i.e. point (i, j) = 4 i + j, output
// channel o = 32 nb + n, input channel c = 8 c8 + 4 h + e at float ((((4 i + j) * NB + nb) * Cin / 8 + c8) * 2 + h) * 128 + 4 n + e.
// Padded output channels are zero.  Returns the float count (out may be NULL to query it) or OFX_EINVAL.
extern "C" long ofx_wino_conv_weight(const float* w, int Cout, int Cin, float* out) {
    OFX_REQUIRE(Cout > 0 && Cin > 0 && Cin % kWBK == 0, OFX_EINVAL);
    const int nb32 = 2 * ((Cout + 63) / 64);
    const long n = 16L * nb32 * 32 * Cin;
    if (!out) return n;
    OFX_REQUIRE(w != nullptr, OFX_EINVAL);
    std::memset(out, 0, (size_t)n * sizeof(float));
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    for (int o = 0; o < Cout; ++o)
        for (int c = 0; c < Cin; ++c) {
            const float* g = w + ((size_t)o * Cin + c) * 9;
            double gg[4][3];   // G g
            for (int i = 0; i < 4; ++i)
                for (int x = 0; x < 3; ++x) gg[i][x] = G[i][0] * g[x] + G[i][1] * g[3 + x] + G[i][2] * g[6 + x];
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) {
                    const double u = gg[i][0] * G[j][0] + gg[i][1] * G[j][1] + gg[i][2] * G[j][2];
                    const long at = ((((long)(4 * i + j) * nb32 + o / 32) * (Cin / 8) + c / 8) * 2 + (c % 8) / 4) * 128 + 4 * (o % 32) + c % 4;
                    out[at] = (float)u;
                }
        }
    return n;
}
