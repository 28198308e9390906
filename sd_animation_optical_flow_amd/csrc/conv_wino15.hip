// Fused 1D Winograd F(4, 5) convolution on the fp32 matrix cores of gfx950: the SepConvGRU's 1x5 and 5x1 layers.
//
// The four per-iteration GRU convolutions (gru.zr1 / q1: 1x5, gru.zr2 / q2: 5x1, 256 input channels) ran on the direct halo-patch
// kernel of conv.hip at ~0.9 of the fp32 MFMA peak; like the 3x3 layers (conv_wino.hip) the only way to take real time off them is
// to execute fewer multiplies.  F(4, 5) produces 4 outputs of a 5-tap filter from 8 inputs with 8 point-wise products per (input,
// output) channel pair: 2 multiplies per output instead of 5.
//
//   y = A^T [ (G g) (.) (B^T d) ]     points {0, 1, -1, 2, -2, 1/2, -1/2, inf}   (Lavin & Gray 2016; Toom-Cook)
//
// Everything between the input and the output stays on chip:
//   * a workgroup owns one 8x16-pixel output patch -- 32 tiles of 1x4 (1x5 layers, along W) or 4x1 (5x1 layers, along H) -- and
//     128 output channels;
//   * per 16-channel slab the input halo (8x20 or 12x16 pixels) is staged in LDS once (buffer descriptors return the zero padding),
//     every thread applies B^T d to one (tile, channel pair) and writes the 8 transformed values to LDS;
//   * wave w owns 32 output channels and ALL 8 points: per point the GEMM [32 tiles x 16 channels] x [16 channels x 32 outputs] on
//     v_mfma_f32_32x32x2_f32 into one 16-register accumulator.  A lane then holds the 8 point values of each of its (tile, channel)
//     elements, so A^T runs in registers and the epilogue starts straight from them: no output exchange through LDS;
//   * the weights U = G g (host, float64, one rounding: ofx_wino15_conv_weight) are stored in the MFMA's B-operand lane order:
//     per point and slab a wave loads two contiguous 1 KB fragments, one slab ahead (64 registers, as the 2D kernel's);
//   * epilogues: plain (scale / shift, addend, ReLU, strided store) and the two GRU gate epilogues with the semantics of
//     igemm_kernel (conv.hip): z = sigmoid -> aux_z, r * h -> aux_rh; h = (1 - z) h + z tanh(.) in place.
// Executed multiplies per output: 8 / 4 = 2 per (cin, cout) against 5 for the direct kernel.
#include "ofx_internal.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

namespace {

constexpr int kWBK = 16;                    // channels per slab
constexpr int kLDV = kWBK + 4;              // transformed tile row stride: conflict-free ds_read_b128 A fragments (as conv_wino.hip)
constexpr int kVF = 8 * 32 * kLDV;          // 5120 floats: [point][tile][channel]
constexpr int kOOB = 0x7FFFFFF0;

// Halo geometry of the two orientations.  VERT = false (1x5): 8 rows x 20 columns, tile t = (row t / 4, column group t % 4) reads
// pixels row * 20 + 4 (t % 4) + 0..7.  VERT = true (5x1): 12 rows x 16 columns, tile t = (row group t / 16, column t % 16) reads
// pixels (4 (t / 16) + 0..7) * 16 + t % 16.  Pixel strides (floats): a half-wave's transform reads (four tiles, 16 floats each) land
// in disjoint banks -- four tiles 4 pixels apart at stride 20 (1x5), 1 pixel apart at stride 16 (5x1).
template <bool VERT> struct Geo {
    static constexpr int W = VERT ? 16 : 20, H = VERT ? 12 : 8;
    static constexpr int pix = W * H;                       // 160 / 192
    static constexpr int items = pix * (kWBK / 4);          // float4 pieces per slab: 640 / 768
    static constexpr int slots = (items + 255) / 256;       // per thread: 3
    static constexpr int ldh = VERT ? 16 : 20;
    static constexpr int tap = VERT ? W : 1;                // pixel step between taps
    static constexpr int halo_f = pix * ldh;                // 3200 / 3072 floats
    static constexpr int smem_f = halo_f + kVF;             // ~33 KB
    __device__ static int tile_base(int t) { return VERT ? (4 * (t >> 4)) * W + (t & 15) : (t >> 2) * W + 4 * (t & 3); }
    // output pixel (dy, dx) in the patch of tile t, output i of the tile
    __device__ static int oy(int t, int i) { return VERT ? 4 * (t >> 4) + i : t >> 2; }
    __device__ static int ox(int t, int i) { return VERT ? (t & 15) : 4 * (t & 3) + i; }
};

struct Wino15K {
    const float* in0;
    const float* in1;
    const float* u;          // ofx_wino15_conv_weight layout
    const float* scale;
    const float* shift;
    const float* addend;
    float* out;
    float* aux_z;
    float* aux_rh;
    float* aux_h;
    int ld0, c0, ld1, cin, ldo, ldadd, ldh;
    int H, W, Cout, act;
    int nblk;                // 128-channel output blocks
    int nb32;                // 32-channel blocks of u
    int tpr, tpi, mtiles;    // patches per image row / per image, patches in all
    int bytes0, bytes1, bytesu;
    float alpha;
};

__device__ __forceinline__ float2 f2(float a, float b) { return make_float2(a, b); }
__device__ __forceinline__ float2 operator+(float2 a, float2 b) { return f2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 operator-(float2 a, float2 b) { return f2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 operator*(float s, float2 a) { return f2(s * a.x, s * a.y); }

template <bool VERT, int EPI>
__global__ __launch_bounds__(256, 2) void wino15_conv_kernel(const Wino15K p) {
    typedef int v4i __attribute__((ext_vector_type(4)));
    using G = Geo<VERT>;
    __shared__ __attribute__((aligned(16))) float smem[G::smem_f];
    float* const Hs = smem;
    float* const Vs = smem + G::halo_f;
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

    // ---- halo staging: item i = (pixel i / 4, float4 slot i % 4) of the slab, pixels row-major over the halo
    const float* in1s = p.in1 ? p.in1 : p.in0;
    const int bytes1s = p.in1 ? p.bytes1 : p.bytes0;
    int hpix[G::slots];
    unsigned hok = 0;
#pragma unroll
    for (int k = 0; k < G::slots; ++k) {
        const int i = tid + 256 * k;
        const int pix = i >> 2;
        const int hy = pix / G::W, hx = pix - hy * G::W;
        const int gy = y0 - (VERT ? 2 : 0) + hy, gx = x0 - (VERT ? 0 : 2) + hx;
        const bool ok = i < G::items && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
        hpix[k] = ok ? (pb * p.H + gy) * p.W + gx : 0;
        hok |= (ok ? 1u : 0u) << k;
    }
    const int hq = (tid & 3) * 16;   // byte offset of this thread's float4 slot (the same for every k)
    float4 pa[G::slots];
    auto a_issue = [&](int cb) __attribute__((always_inline)) {
        const int c = cb * kWBK;
        const bool s0 = c < p.c0;    // wave-uniform
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(s0 ? p.in0 : in1s), (short)0, s0 ? p.bytes0 : bytes1s, 0x00020000);
        const int so = (s0 ? c : c - p.c0) * 4;
        const int ldb = (s0 ? p.ld0 : p.ld1) * 4;
#pragma unroll
        for (int k = 0; k < G::slots; ++k) {
            const int vo = ((hok >> k) & 1u) ? hpix[k] * ldb + hq : kOOB;
            v4i t = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, so, 0);
            pa[k] = *reinterpret_cast<float4*>(&t);
        }
    };

    // ---- weights: point q, 32-channel block 4 nb + wave, 8-channel chunk 2 cb + ks -> one contiguous 1 KB fragment
    const __amdgpu_buffer_rsrc_t rsu = __builtin_amdgcn_make_buffer_rsrc((void*)p.u, (short)0, p.bytesu, 0x00020000);
    const int c8n = p.cin >> 3;
    const int wlane = lane * 16;
    const int nb32 = 4 * nb + wave;
    float4 wr[8][2];
    auto w_issue = [&](int q, int cb) __attribute__((always_inline)) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int so = ((q * p.nb32 + nb32) * c8n + 2 * cb + ks) * 1024;   // scalar
            v4i t = __builtin_amdgcn_raw_buffer_load_b128(rsu, wlane, so, 0);
            wr[q][ks] = *reinterpret_cast<float4*>(&t);
        }
    };

    f32x16 acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[q][e] = 0.f;

    // input transform: thread = (tile tid / 8, channel pair tid % 8)
    const int ttile = tid >> 3, tcp = tid & 7;
    const float* const tsrc = Hs + G::tile_base(ttile) * G::ldh + 2 * tcp;
    float* const tdst = Vs + ttile * kLDV + 2 * tcp;
    // A fragment: tile = lane & 31, channels 8 ks + 4 (lane >> 5) + 0..3 (the k order the weights are stored in)
    const float* const afrag = Vs + (lane & 31) * kLDV + 4 * (lane >> 5);

    const int CB = p.cin / kWBK;
    a_issue(0);
#pragma unroll
    for (int q = 0; q < 8; ++q) w_issue(q, 0);
    for (int cb = 0; cb < CB; ++cb) {
        const int nx = cb + 1 < CB ? cb + 1 : cb;   // the last slab re-issues itself: no branch, loads stay in bounds
#pragma unroll
        for (int k = 0; k < G::slots; ++k) {
            const int i = tid + 256 * k;
            if (G::slots * 256 > G::items && k == G::slots - 1 && i >= G::items) break;
            *reinterpret_cast<float4*>(&Hs[(i >> 2) * G::ldh + (i & 3) * 4]) = pa[k];
        }
        __syncthreads();
        {
            float2 d[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] = *reinterpret_cast<const float2*>(tsrc + j * G::tap * G::ldh);
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
            for (int j = 0; j < 8; ++j) *reinterpret_cast<float2*>(tdst + j * 32 * kLDV) = v[j];
        }
        __syncthreads();
        a_issue(nx);   // the next slab's halo lands during this slab's products (issued here, not live across the transform)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const float4 a = *reinterpret_cast<const float4*>(afrag + q * 32 * kLDV + 8 * ks);
                const float4 b = wr[q][ks];
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc[q], 0, 0, 0);
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc[q], 0, 0, 0);
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc[q], 0, 0, 0);
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc[q], 0, 0, 0);
            }
            w_issue(q, nx);   // this point's fragments for the next slab: the rest of the slab hides the load
        }
    }

    // ---- output transform in registers, then the epilogue.  Element e of the C layout: tile (e & 3) + 8 (e >> 2) + 4 (lane >> 5),
    // output channel lane & 31 of the wave's 32.
    const int n = nb * 128 + wave * 32 + (lane & 31);
    if (n >= p.Cout) return;   // no barrier follows
    const float sc = (p.scale ? p.scale[n] : 1.0f) * p.alpha;
    const float sh = p.shift ? p.shift[n] : 0.0f;
    const float act_lo = p.act == OFX_ACT_RELU ? 0.0f : -3.402823466e38f;
    const int hd = p.Cout >> 1;
    const bool r_half = EPI == OFX_EPI_GRU_ZR && nb * 128 >= hd;   // block-uniform (fits: hd % 128 == 0)
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
            for (int i = 0; i < 4; ++i) pix[u][i] = ((long)pb * p.H + y0 + G::oy(tile, i)) * p.W + x0 + G::ox(tile, i);
            const float m0 = acc[0][e], m1 = acc[1][e], m2 = acc[2][e], m3 = acc[3][e];
            const float m4 = acc[4][e], m5 = acc[5][e], m6 = acc[6][e], m7 = acc[7][e];
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

template <bool VERT>
int launch_epi(const Wino15K& k, int epi, dim3 grid, dim3 block, hipStream_t s) {
    switch (epi) {
        case OFX_EPI_PLAIN: OFX_LAUNCH((wino15_conv_kernel<VERT, OFX_EPI_PLAIN>), grid, block, s, k); break;
        case OFX_EPI_GRU_ZR: OFX_LAUNCH((wino15_conv_kernel<VERT, OFX_EPI_GRU_ZR>), grid, block, s, k); break;
        case OFX_EPI_GRU_Q: OFX_LAUNCH((wino15_conv_kernel<VERT, OFX_EPI_GRU_Q>), grid, block, s, k); break;
        default: return OFX_EINVAL;
    }
    return ofx_launch_status();
}

}  // namespace

// Shape test for the fused kernel: fp32, one problem, stride-1 1x5 (pad 0, 2) or 5x1 (pad 2, 0) keeping the map size, a map of
// whole 8x16 patches, 16-channel slabs that never straddle the two input segments; the plain epilogue (ReLU or identity, optional
// addend, no fused norm or residual) or a GRU gate epilogue whose z | r split falls on a 128-channel block boundary.
bool ofx_conv_wino15_fits(const ofx_conv_desc* d) {
    const int cin = d->c0 + d->c1;
    const bool shape = (d->KH == 1 && d->KW == 5 && d->padH == 0 && d->padW == 2) || (d->KH == 5 && d->KW == 1 && d->padH == 2 && d->padW == 0);
    bool epi = false;
    switch (d->epi) {
        case OFX_EPI_PLAIN: epi = d->out != nullptr && d->ldo >= d->Cout && (d->act == OFX_ACT_NONE || d->act == OFX_ACT_RELU); break;
        case OFX_EPI_GRU_ZR: epi = (d->Cout / 2) % 128 == 0; break;
        case OFX_EPI_GRU_Q: epi = true; break;
        default: break;
    }
    return d->precision == OFX_PREC_FP32 && (d->nz <= 1) && shape && d->stride == 1 && d->Hout == d->Hin && d->Wout == d->Win &&
           d->Hin % 8 == 0 && d->Win % 16 == 0 && cin % kWBK == 0 && d->c0 % kWBK == 0 && epi && !d->nmean && !d->res &&
           d->wino_w != nullptr && ofx_aligned16(d->wino_w);
}

long ofx_conv_wino15_patches(const ofx_conv_desc* d) {
    return (long)d->B * (d->Hin / 8) * (d->Win / 16);
}

// Multiplies the fused kernel executes for `d` (x 2 FLOPs): 8 point products per 4-output tile, input channel and output channel
double ofx_conv_wino15_flops(const ofx_conv_desc* d) {
    return 2.0 * 8.0 * ((double)d->B * d->Hout * d->Wout / 4.0) * (double)(d->c0 + d->c1) * d->Cout;
}

// The caller has validated the descriptor (ofx_conv2d_alpha) and ofx_conv_wino15_fits(d).
int ofx_conv_wino15_launch(const ofx_conv_desc* d, float alpha, hipStream_t s) {
    Wino15K k;
    k.in0 = d->in0; k.in1 = d->in1; k.u = d->wino_w; k.scale = d->scale; k.shift = d->shift; k.addend = d->addend; k.out = d->out;
    k.aux_z = d->aux_z; k.aux_rh = d->aux_rh; k.aux_h = d->aux_h;
    k.ld0 = d->ld0; k.c0 = d->c0; k.ld1 = d->ld1; k.cin = d->c0 + d->c1; k.ldo = d->ldo; k.ldadd = d->ldadd; k.ldh = d->ldh;
    k.H = d->Hin; k.W = d->Win; k.Cout = d->Cout; k.act = d->act;
    k.nblk = (d->Cout + 127) / 128;
    k.nb32 = 4 * k.nblk;
    k.tpr = d->Win / 16;
    k.tpi = (d->Hin / 8) * k.tpr;
    const long mtiles = (long)d->B * k.tpi;
    const long npix = (long)d->B * d->Hin * d->Win;
    const long ext0 = ((npix - 1) * d->ld0 + d->c0) * 4, ext1 = d->in1 ? ((npix - 1) * d->ld1 + d->c1) * 4 : 0;
    const long extu = 8L * k.nb32 * 32 * k.cin * 4;
    OFX_REQUIRE(ext0 < (1L << 31) - 64 && ext1 < (1L << 31) - 64 && extu < (1L << 31) - 64, OFX_EINVAL);
    OFX_REQUIRE(mtiles * k.nblk < (1L << 31), OFX_EINVAL);
    k.mtiles = (int)mtiles;
    k.bytes0 = (int)ext0; k.bytes1 = (int)ext1; k.bytesu = (int)extu;
    k.alpha = alpha;
    const dim3 grid((unsigned)(k.mtiles * k.nblk), 1, 1), block(256, 1, 1);
    return d->KH == 5 ? launch_epi<true>(k, d->epi, grid, block, s) : launch_epi<false>(k, d->epi, grid, block, s);
}

// Host: OIHW 1x5 or 5x1 weights -> U = G g per (output, input) channel pair in float64, rounded once to fp32, in the fused kernel's
// operand order: [8 points][Cout rounded up to 128, as 32-channel blocks][Cin / 8][2][32][4], i.e. point q, output channel
// o = 32 nb + n, input channel c = 8 c8 + 4 h + e at float (((q * NB + nb) * Cin / 8 + c8) * 2 + h) * 128 + 4 n + e.  G rows: the
// points 0, 1, -1, 2, -2, 1/2, -1/2 scaled by 1 / prod_{k != j} (a_j - a_k) (row 0 sign-flipped, with B^T's), and inf.  Padded
// output channels are zero.  Returns the float count (out may be NULL to query it) or OFX_EINVAL.
extern "C" long ofx_wino15_conv_weight(const float* w, int Cout, int Cin, int KH, int KW, float* out) {
    OFX_REQUIRE(Cout > 0 && Cin > 0 && Cin % kWBK == 0 && ((KH == 1 && KW == 5) || (KH == 5 && KW == 1)), OFX_EINVAL);
    const int nb32 = 4 * ((Cout + 127) / 128);
    const long n = 8L * nb32 * 32 * Cin;
    if (!out) return n;
    OFX_REQUIRE(w != nullptr, OFX_EINVAL);
    std::memset(out, 0, (size_t)n * sizeof(float));
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
    for (int o = 0; o < Cout; ++o)
        for (int c = 0; c < Cin; ++c) {
            const float* g = w + ((size_t)o * Cin + c) * 5;   // the 5 taps are contiguous in either orientation
            for (int q = 0; q < 8; ++q) {
                double u = 0.0;
                for (int t = 0; t < 5; ++t) u += G[q][t] * (double)g[t];
                const long at = ((((long)q * nb32 + o / 32) * (Cin / 8) + c / 8) * 2 + (c % 8) / 4) * 128 + 4 * (o % 32) + c % 4;
                out[at] = (float)u;
            }
        }
    return n;
}
