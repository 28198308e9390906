// The hint stem of ControlNet (controlnet.py:164-180, `input_hint_block`): eight 3x3 convolutions, padding 1, strides
// 1,1,2,1,2,1,2,1, channels hint -> 16 -> 16 -> 32 -> 32 -> 96 -> 96 -> 256 -> model_channels, nn.SiLU after all but the last.
//
//   ofx_conv3x3_silu   out = silu(conv3x3(x, pad 1, stride 1 | 2) + bias) on NHWC fp32, exact fp32 on v_mfma_f32_16x16x4_f32
//
// ofx_conv2d's tiles are built around 64 output channels and its activations know no SiLU; here the N side of the matrix
// instruction is 16 channels, so the 16- and 32-channel layers at image resolution fill it.  One workgroup (four waves) owns an
// 8 x 16 tile of output pixels and BN = 16 NSUB output channels of one image:
//   * output pixels on the M side: one MFMA row block is the 16 pixels of one tile row, a wave owns two tile rows and all NSUB
//     channel blocks (2 NSUB accumulators of 4 registers);
//   * the input channels are walked in chunks of KC (8, or 4 when Cin % 8 != 0).  Per chunk the halo patch of the tile --
//     (7 S + 3) x (15 S + 3) pixels, zeros outside the image -- goes to LDS channel-major (a plane per channel, so the 16 lanes of
//     an A operand read consecutive words at stride 1) and the chunk's weights go to LDS as [tap][channel][BN] (the 16 lanes of
//     a B operand read consecutive words): each weight is read from memory once per workgroup.  The next chunk's loads are
//     issued into registers before the current chunk is multiplied and written to LDS after it;
//   * the K order of the accumulation is (chunk, ky, kx, channel), in two levels: the 9 KC products of a chunk are one fp32 fused
//     multiply-add chain from zero, and the chunk sums are added in order -- Cin / KC additions.  A single chain over the 2304
//     products of the 256-channel layer drifts further from float64 than a blocked fp32 sum does (the stem
//     of the test configuration missed its bar that way); then + bias, then y * ofx_sigmoid(y).
// Plane and row strides of the two LDS images are 16 or 48 modulo 64 words, which spreads the four k-lanes of an operand over the
// banks (conflict-free at stride 1, two-way at stride 2, where the pixel lanes are two words apart).
// Addresses are 64-bit; pixel and tile counts are 32-bit ints (checked by the launcher).
#include "ofx_internal.h"

namespace {

constexpr int kTH = 8, kTW = 16;          // output pixels of a workgroup tile: rows x columns (columns = the MFMA's M)

struct CnK {
    const float* x;
    const float* w;
    const float* bias;
    float* out;
    int ldx, ldw, ldo, Cin, Cout, H, W, Ho, Wo, tiles_x, tiles_y, silu;
};

template <int S, int KC, int NSUB>
__global__ __launch_bounds__(256) void conv3x3_silu_kernel(CnK k) {
    constexpr int PH = (kTH - 1) * S + 3, PW = (kTW - 1) * S + 3, NPIX = PH * PW;
    constexpr int PLANE = (NPIX + 63) / 64 * 64 + 16;
    constexpr int BN = NSUB * 16, BNP = BN == 16 ? 16 : BN + 16;
    __shared__ float xs[KC * PLANE];
    __shared__ float ws[9 * KC * BNP];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, kq = lane >> 4;
    int t = blockIdx.x;
    const int tx = t % k.tiles_x;
    t /= k.tiles_x;
    const int ty = t % k.tiles_y, b = t / k.tiles_y;
    const int oy0 = ty * kTH, ox0 = tx * kTW, n0 = blockIdx.y * BN;
    const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
    const float* xb = k.x + (size_t)b * k.H * k.W * k.ldx;

    f32x4 acc[2][NSUB];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int ns = 0; ns < NSUB; ++ns) acc[r][ns] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the staging of a chunk in two halves: its float4s come from memory into registers while the chunk before it is multiplied,
    // and go to LDS between the two barriers.  Item i of the patch is (pixel i % NPIX, channel quad i / NPIX), item i of the weights
    // (channel o = i % BN, quad q, tap); consecutive lanes write consecutive LDS words.
    constexpr int XN = NPIX * (KC / 4), WN = BN * 9 * (KC / 4), XI = (XN + 255) / 256, WI = (WN + 255) / 256;
    float4 xr[XI], wr[WI];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int j = 0; j < XI; ++j) {
            const int i = tid + j * 256;
            const int pix = i % NPIX, q = i / NPIX;
            const int iy = iy0 + pix / PW, ix = ix0 + pix % PW;
            xr[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < XN && iy >= 0 && iy < k.H && ix >= 0 && ix < k.W)
                xr[j] = *reinterpret_cast<const float4*>(xb + ((size_t)iy * k.W + ix) * k.ldx + c0 + q * 4);
        }
#pragma unroll
        for (int j = 0; j < WI; ++j) {
            const int i = tid + j * 256;
            const int o = i % BN, rest = i / BN;
            const int q = rest % (KC / 4), tap = rest / (KC / 4);
            wr[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < WN) wr[j] = *reinterpret_cast<const float4*>(k.w + (size_t)(n0 + o) * k.ldw + (size_t)tap * k.Cin + c0 + q * 4);
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < k.Cin; c0 += KC) {
        __syncthreads();                                       // the previous chunk's operands are no longer read
#pragma unroll
        for (int j = 0; j < XI; ++j) {
            const int i = tid + j * 256;
            if (i >= XN) break;
            float* d = xs + (i / NPIX * 4) * PLANE + i % NPIX;
            d[0] = xr[j].x; d[PLANE] = xr[j].y; d[2 * PLANE] = xr[j].z; d[3 * PLANE] = xr[j].w;
        }
#pragma unroll
        for (int j = 0; j < WI; ++j) {
            const int i = tid + j * 256;
            if (i >= WN) break;
            const int o = i % BN, rest = i / BN;
            float* d = ws + (rest / (KC / 4) * KC + rest % (KC / 4) * 4) * BNP + o;
            d[0] = wr[j].x; d[BNP] = wr[j].y; d[2 * BNP] = wr[j].z; d[3 * BNP] = wr[j].w;
        }
        __syncthreads();
        if (c0 + KC < k.Cin) fetch(c0 + KC);                   // in flight under this chunk's MFMAs
        f32x4 part[2][NSUB];                                   // this chunk's 9 KC products, summed on their own (header)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int ns = 0; ns < NSUB; ++ns) part[r][ns] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int k4 = 0; k4 < KC / 4; ++k4) {
                    const float* xp = xs + (k4 * 4 + kq) * PLANE + kx + m * S;
                    const float a0 = xp[((wave * 2) * S + ky) * PW];
                    const float a1 = xp[((wave * 2 + 1) * S + ky) * PW];
                    const float* wp = ws + ((ky * 3 + kx) * KC + k4 * 4 + kq) * BNP + m;
#pragma unroll
                    for (int ns = 0; ns < NSUB; ++ns) {
                        const float bv = wp[ns * 16];
                        part[0][ns] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv, part[0][ns], 0, 0, 0);
                        part[1][ns] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv, part[1][ns], 0, 0, 0);
                    }
                }
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int ns = 0; ns < NSUB; ++ns) acc[r][ns] += part[r][ns];
    }
    // C/D of the 16x16 forms: column (channel) = lane & 15, row (pixel of the tile row) = 4 (lane >> 4) + register
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int oy = oy0 + wave * 2 + r;
        if (oy >= k.Ho) continue;
        float* orow = k.out + ((size_t)b * k.Ho + oy) * k.Wo * k.ldo;
#pragma unroll
        for (int ns = 0; ns < NSUB; ++ns) {
            const int n = n0 + ns * 16 + m;
            const float bs = k.bias ? k.bias[n] : 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ox = ox0 + kq * 4 + j;
                if (ox >= k.Wo) continue;
                float y = acc[r][ns][j] + bs;
                if (k.silu) y = y * ofx_sigmoid(y);
                orow[(size_t)ox * k.ldo + n] = y;
            }
        }
    }
}

template <int S, int KC>
static void launch_nsub(int nsub, dim3 grid, hipStream_t s, const CnK& k) {
    const dim3 block(256, 1, 1);
    switch (nsub) {
        case 1: hipLaunchKernelGGL((conv3x3_silu_kernel<S, KC, 1>), grid, block, 0, s, k); break;
        case 2: hipLaunchKernelGGL((conv3x3_silu_kernel<S, KC, 2>), grid, block, 0, s, k); break;
        case 4: hipLaunchKernelGGL((conv3x3_silu_kernel<S, KC, 4>), grid, block, 0, s, k); break;
        default: hipLaunchKernelGGL((conv3x3_silu_kernel<S, KC, 6>), grid, block, 0, s, k); break;
    }
}

}  // namespace

// w is `ofx_pack_conv_weight`'s operand with cin_pad = Cin: w[o * ldw + (ky * 3 + kx) * Cin + c], ldw >= 9 Cin (its Kpad).
extern "C" int ofx_conv3x3_silu(const float* x, int ldx, int Cin, const float* w, int ldw, const float* bias, float* out, int ldo,
                                int Cout, int B, int H, int W, int stride, int silu, void* stream) {
    OFX_REQUIRE(x && w && out, OFX_EINVAL);
    OFX_REQUIRE(stride == 1 || stride == 2, OFX_EINVAL);
    OFX_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, OFX_EINVAL);
    OFX_REQUIRE(Cin % 4 == 0 && Cout % 16 == 0, OFX_EINVAL);
    OFX_REQUIRE(ldx >= Cin && ldo >= Cout && (long)ldw >= 9L * Cin, OFX_EINVAL);
    OFX_REQUIRE(ldx % 4 == 0 && ldo % 4 == 0 && ldw % 4 == 0, OFX_EALIGN);
    OFX_REQUIRE(ofx_aligned16(x) && ofx_aligned16(w) && ofx_aligned16(out) && (!bias || (((uintptr_t)bias) & 3u) == 0), OFX_EALIGN);
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    // pixels and tiles are 32-bit ints in the kernel (addresses are 64-bit)
    OFX_REQUIRE((long)B * H * W < (1L << 31), OFX_EINVAL);
    const int nsub = Cout % 64 == 0 ? 4 : Cout % 96 == 0 ? 6 : Cout % 32 == 0 ? 2 : 1;
    const int ntiles = Cout / (16 * nsub);
    CnK k;
    k.x = x; k.w = w; k.bias = bias; k.out = out;
    k.ldx = ldx; k.ldw = ldw; k.ldo = ldo; k.Cin = Cin; k.Cout = Cout; k.H = H; k.W = W; k.Ho = Ho; k.Wo = Wo;
    k.tiles_x = (Wo + kTW - 1) / kTW;
    k.tiles_y = (Ho + kTH - 1) / kTH;
    k.silu = silu ? 1 : 0;
    const long tiles = (long)B * k.tiles_y * k.tiles_x;
    OFX_REQUIRE(tiles < (1L << 31) && ntiles <= 65535, OFX_EINVAL);
    hipStream_t s = (hipStream_t)stream;
    OfxProfScope prof("conv3x3_silu", s);
    prof.flops(2.0 * 9.0 * (double)B * Ho * Wo * Cin * Cout);
    const dim3 grid((unsigned)tiles, (unsigned)ntiles, 1);
    if (stride == 1) {
        if (Cin % 8 == 0) launch_nsub<1, 8>(nsub, grid, s, k);
        else launch_nsub<1, 4>(nsub, grid, s, k);
    } else {
        if (Cin % 8 == 0) launch_nsub<2, 8>(nsub, grid, s, k);
        else launch_nsub<2, 4>(nsub, grid, s, k);
    }
    return ofx_launch_status();
}
