// First-stage (VAE) decoder pieces that the convolution / norm / attention kernels do not cover
// (ldm/modules/diffusionmodules/model.py:43-58 `Upsample`, ofgen_keyframe_inpaint.py:234-235 `decode_latent`):
//
//   ofx_upconv2x              conv3x3(pad 1)(interpolate(x, 2x, nearest)) without the upsampled map: output pixel (2y + py, 2x + px)
//                             sees only the 2x2 low-resolution neighbourhood rows {y - 1 + py, y + py} x columns {x - 1 + px, x + px},
//                             with the 3x3 taps that land on the same low-resolution pixel added up beforehand
//                             (ofx_upconv2x_weight).  Four implicit GEMMs (one per parity, blockIdx.y) of M = B*H*W low-resolution
//                             pixels, N = Cout, K = 4 * Cin on v_mfma_f32_32x32x2_f32; each scatters its rows to its parity of the
//                             [B,2H,2W] map.  4 taps per output instead of 9, and the 4x larger map is written once, never read.
//   ofx_upconv2x_prec         the same with the arithmetic chosen: OFX_PREC_FP32 calls through; OFX_PREC_F16 rounds both operands to
//                             fp16 as they are staged and contracts them on v_mfma_f32_32x32x16_f16 (fp32 accumulate, bias and store)
//   ofx_upsample2x_nearest_f32  the materialising upsample (the unfused pair's first half)
//   ofx_decode_to_u8          f32 RGB in [-1,1] -> u8 BGR, the bits of the reference's numpy expression
//
// The GEMM follows conv.hip's general schedule in its plainest form: 256 threads = 2x2 waves, a 128 x BN tile (BN = 128, or 64 for
// narrow layers), 16-wide K chunks staged k-contiguous in LDS with a 20-float row stride (conflict-free ds_read_b128 fragments, one
// read feeding four MFMAs; lane half h supplies k = 8 ks + 4 h + s to MFMA s -- the same permutation on both operands), two LDS
// stages, one barrier per chunk, the next chunk's global loads in flight during the MFMA block.  Addresses are 64-bit; rows past M /
// Cout, taps in the zero padding and channels past Cin stage zeros.
#include "ofx_internal.h"

#include <algorithm>
#include <cstdlib>

namespace {

constexpr int kBK = 16;            // K chunk
constexpr int kLDK = kBK + 4;      // LDS row stride in floats
constexpr int kBKh = 32;           // K chunk of the fp16 form (the convolution family's rule off the halo patch)
constexpr int kRowBh = kBKh * 2 + 16;   // its LDS row in bytes: 32 halves + 16 bytes of padding (conv.hip, ROWB)

struct UpK {
    const float* x;
    const float* w;                // [4 parities][Cout][4 taps][Cin]
    const float* bias;
    float* out;
    int B, H, W, Cin, Cout, ldo;
    int M;                         // B * H * W
    int ntiles;
    int cchunks;                   // ceil(Cin / 16); fp16: ceil(Cin / 32)
};

// PREC = OFX_PREC_F16: the arithmetic of conv.hip's fp16 kernels on the same problem.  Both operands stay fp32 in memory and are
// rounded fp32 -> fp16 (nearest even, v_cvt_pk_f16_f32) as they are committed to LDS; 32 channels of a tap per chunk, rows of 80
// bytes written 8 bytes per float4 slot; a fragment is one ds_read_b128 (lane l: row l & 31, the eight consecutive k of group
// l >> 5 -- the same on both operands), ONE v_mfma_f32_32x32x16_f16 per (i, j) and 16 k, fp32 accumulate.  Loads, guards, pipeline
// and epilogue are the fp32 form's.
// PREC = OFX_PREC_F16_W: the same with the folded weights stored in half (ofx_half_conv_weight): 8-byte loads of four halves,
// committed as loaded -- the same LDS contents, so the same bits out.
// (the 128 x 64 tile on half weights asks for the five waves per SIMD its fp32-weight twin reaches on its own: left alone it compiles
// to 8 registers more and four waves; every other instantiation keeps the default)
template <int BN, int PREC = OFX_PREC_FP32>
__global__ __launch_bounds__(256, (PREC == OFX_PREC_F16_W && BN == 64) ? 5 : 1) void upconv2x_kernel(const UpK p) {
    constexpr bool F16W = PREC == OFX_PREC_F16_W;     // the folded weights are halves in memory: 8-byte loads, committed as they are
    constexpr bool F16 = PREC == OFX_PREC_F16 || F16W;
    static_assert(F16 || PREC == OFX_PREC_FP32, "fp32 or fp16");
    constexpr int BM = 128, WM = 64, WN = BN / 2, TM = WM / 32, TN = WN / 32;
    constexpr int BK = F16 ? kBKh : kBK;
    constexpr int QPR = BK / 4;                       // float4 slots per staged row
    constexpr int RPG = 256 / QPR;                    // rows per pass of the 256 threads: 64, fp16 32
    constexpr int A_PER = BM / RPG, B_PER = BN / RPG;
    constexpr int STAGE = F16 ? (BM + BN) * (kRowBh / 4) : (BM + BN) * kLDK;   // floats
    __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int nt = blockIdx.x % p.ntiles, mt = blockIdx.x / p.ntiles;
    const int par = blockIdx.y, py = par >> 1, px = par & 1;
    const int m0 = mt * BM, n0 = nt * BN;

    // staging role: float4 slot kq of rows r0 + RPG i; rows permuted inside groups of 16 so that one ds_write_b128 pass
    // (16 lanes) covers 16 distinct 16-byte bank groups (conv.hip, r0).  fp16: 8-byte writes, 32 lanes per pass, the rows of one
    // pass every 4th row (80-byte rows then start 32 bytes apart modulo 256)
    const int kq = tid % QPR, j0 = tid / QPR;
    const int r0 = F16 ? 16 * (j0 >> 4) + 4 * (j0 & 3) + ((j0 >> 2) & 3) : (j0 & 3) * 4 + ((j0 >> 2) & 3) + (j0 >> 4) * 16;
    const int HW = p.H * p.W;
    int a_b[A_PER], a_y[A_PER], a_x[A_PER];
    bool a_ok[A_PER];
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
        const int m = m0 + r0 + RPG * i;
        a_ok[i] = m < p.M;
        const int mm = a_ok[i] ? m : 0;
        a_b[i] = mm / HW;
        const int rem = mm - a_b[i] * HW;
        a_y[i] = rem / p.W;
        a_x[i] = rem - a_y[i] * p.W;
    }
    const size_t wrow = (size_t)4 * p.Cin;            // floats per output channel of one parity
    const float* wpar = p.w + (size_t)par * p.Cout * wrow;
    const _Float16* wparh = reinterpret_cast<const _Float16*>(p.w) + (size_t)par * p.Cout * wrow;   // F16W: the same element, two bytes each

    typedef float f32x2_ __attribute__((ext_vector_type(2)));
    f32x4 ra[A_PER], rb[F16W ? 1 : B_PER];    // native vectors: a select between two of them stays in registers
    f32x2_ rh[F16W ? B_PER : 1];              // half weights: four halves per slot
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const f32x2_ zero2 = {0.f, 0.f};
    // branch-free: a lane whose float4 does not exist reads the first 16 bytes of the operand instead and keeps zeros
    auto load = [&](int t, int cb) __attribute__((always_inline)) {
        const int ty = t >> 1, tx = t & 1;
        const int c = cb * BK + kq * 4;
        const bool cok = c < p.Cin;                   // Cin % 4 == 0: a float4 is inside or outside as a whole
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            const int iy = a_y[i] - 1 + py + ty, ix = a_x[i] - 1 + px + tx;
            const bool ok = cok && a_ok[i] && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
            const f32x4 v = *reinterpret_cast<const f32x4*>(ok ? p.x + (((size_t)a_b[i] * p.H + iy) * p.W + ix) * p.Cin + c : p.x);
            ra[i] = ok ? v : zero4;
        }
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            const int n = n0 + r0 + RPG * i;
            const bool ok = cok && n < p.Cout;
            if constexpr (F16W) {   // the same element index, two bytes per element (Cin % 4 == 0: 8-byte aligned)
                const f32x2_ v = *reinterpret_cast<const f32x2_*>(ok ? wparh + (size_t)n * wrow + (size_t)t * p.Cin + c : reinterpret_cast<const _Float16*>(p.w));
                rh[i] = ok ? v : zero2;
            } else {
                const f32x4 v = *reinterpret_cast<const f32x4*>(ok ? wpar + (size_t)n * wrow + (size_t)t * p.Cin + c : p.w);
                rb[i] = ok ? v : zero4;
            }
        }
    };
    auto commit = [&](float* st) __attribute__((always_inline)) {
        if constexpr (F16) {
            // fp32 -> fp16, round-to-nearest-even; beyond +-65504 the result is an infinity (conv.hip, cvt_store)
            typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
            char* a0 = reinterpret_cast<char*>(st);
            char* b0 = a0 + BM * kRowBh;
#pragma unroll
            for (int i = 0; i < A_PER; ++i) *reinterpret_cast<f16x4*>(a0 + (r0 + RPG * i) * kRowBh + kq * 8) = __builtin_convertvector(ra[i], f16x4);
#pragma unroll
            for (int i = 0; i < B_PER; ++i) {
                if constexpr (F16W) *reinterpret_cast<f32x2_*>(b0 + (r0 + RPG * i) * kRowBh + kq * 8) = rh[i];
                else *reinterpret_cast<f16x4*>(b0 + (r0 + RPG * i) * kRowBh + kq * 8) = __builtin_convertvector(rb[i], f16x4);
            }
        } else {
#pragma unroll
            for (int i = 0; i < A_PER; ++i) *reinterpret_cast<f32x4*>(st + (r0 + RPG * i) * kLDK + kq * 4) = ra[i];
#pragma unroll
            for (int i = 0; i < B_PER; ++i) *reinterpret_cast<f32x4*>(st + (BM + r0 + RPG * i) * kLDK + kq * 4) = rb[i];
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int NK = 4 * p.cchunks;
    int t_next = 0, cb_next = 0;
    auto advance = [&]() __attribute__((always_inline)) {
        if (++cb_next == p.cchunks) { cb_next = 0; ++t_next; }
    };
    load(t_next, cb_next);
    advance();
    commit(smem);
    __syncthreads();
    const int frow = lane & 31, fk = (lane >> 5) * 4;
    for (int kt = 0; kt < NK; ++kt) {
        const bool more = kt + 1 < NK;
        if (more) {
            load(t_next, cb_next);
            advance();
        }
        if constexpr (F16) {
            typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
            const char* a0 = reinterpret_cast<const char*>(smem + (kt & 1) * STAGE);
            const char* b0 = a0 + BM * kRowBh;
#pragma unroll
            for (int ks = 0; ks < BK / 16; ++ks) {
                f16x8 a[TM], b[TN];
                const int ko = ks * 32 + (lane >> 5) * 16;                    // bytes: halves 16 ks + 8 (lane >> 5) .. + 7
#pragma unroll
                for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const f16x8*>(a0 + (wm * WM + i * 32 + frow) * kRowBh + ko);
#pragma unroll
                for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const f16x8*>(b0 + (wn * WN + j * 32 + frow) * kRowBh + ko);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        } else {
            const float* As = smem + (kt & 1) * STAGE;
            const float* Bs = As + BM * kLDK;
#pragma unroll
            for (int ks = 0; ks < kBK / 8; ++ks) {
                f32x4 a[TM], b[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const f32x4*>(As + (wm * WM + i * 32 + frow) * kLDK + ks * 8 + fk);
#pragma unroll
                for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const f32x4*>(Bs + (wn * WN + j * 32 + frow) * kLDK + ks * 8 + fk);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b[j].x, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b[j].y, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, b[j].z, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, b[j].w, acc[i][j], 0, 0, 0);
                    }
            }
        }
        if (more) commit(smem + ((kt + 1) & 1) * STAGE);
        __syncthreads();
    }

    // epilogue.  C layout of the 32x32 MFMA: column n = lane & 31, row m = (e & 3) + 8 (e >> 2) + 4 (lane >> 5).  Row m is the
    // low-resolution pixel (b, y, x); it lands on pixel (2y + py, 2x + px) of the [B, 2H, 2W] map.
    const int H2 = 2 * p.H, W2 = 2 * p.W;
    int ncol[TN];
    float bv[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        ncol[j] = n0 + wn * WN + j * 32 + (lane & 31);
        bv[j] = (p.bias && ncol[j] < p.Cout) ? p.bias[ncol[j]] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = m0 + wm * WM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
            if (m >= p.M) continue;
            const int b = m / HW;
            const int rem = m - b * HW;
            const int y = rem / p.W, x = rem - y * p.W;
            float* orow = p.out + (((size_t)b * H2 + 2 * y + py) * W2 + 2 * x + px) * p.ldo;
#pragma unroll
            for (int j = 0; j < TN; ++j)
                if (ncol[j] < p.Cout) orow[ncol[j]] = acc[i][j][e] + bv[j];
        }
}

// out[b, Y, X, :] = in[b, Y / 2, X / 2, :], float4 per thread
__global__ __launch_bounds__(256) void upsample2x_kernel(const float4* __restrict__ in, float4* __restrict__ out, int H, int W, int C4, size_t total) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int W2 = 2 * W, H2 = 2 * H;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int c = (int)(i % C4);
        const size_t pix = i / C4;
        const int X = (int)(pix % W2);
        const size_t rest = pix / W2;
        const int Y = (int)(rest % H2);
        const size_t b = rest / H2;
        out[i] = in[((b * H + (Y >> 1)) * W + (X >> 1)) * C4 + c];
    }
}

// (clip(x, -1, 1) * 127.5 + 127.5) truncated: the product and the sum are rounded separately, as numpy does.  Contraction is switched
// off for this function: the __fmul_rn / __fadd_rn intrinsics are plain operators here and would fuse into one v_fma_f32, which
// lands on the other byte for values next to a byte boundary.
__device__ __forceinline__ unsigned dec_byte(float v) {
#pragma clang fp contract(off)
    v = fminf(fmaxf(v, -1.0f), 1.0f);
    const float prod = v * 127.5f;
    const float sum = prod + 127.5f;
    return (unsigned)(int)sum;
}

// four pixels per thread: 12 output bytes as three 32-bit words (BGR BGR BGR BGR); the last, short group byte by byte
__global__ __launch_bounds__(256) void decode_to_u8_kernel(const float* __restrict__ x, int ld, uint8_t* __restrict__ out, size_t npix) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t p0 = g * 4;
    if (p0 >= npix) return;
    unsigned by[12];
    const int cnt = (int)(npix - p0 < 4 ? npix - p0 : 4);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float* px = x + (p0 + (q < cnt ? q : 0)) * ld;
        by[3 * q + 0] = dec_byte(px[2]);
        by[3 * q + 1] = dec_byte(px[1]);
        by[3 * q + 2] = dec_byte(px[0]);
    }
    if (cnt == 4) {
        uint32_t* o = reinterpret_cast<uint32_t*>(out + p0 * 3);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = by[4 * k] | (by[4 * k + 1] << 8) | (by[4 * k + 2] << 16) | (by[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 3 * cnt; ++k) out[p0 * 3 + k] = (uint8_t)by[k];
    }
}

}  // namespace

// Operand order: out[((p * Cout + o) * 4 + t) * Cin + c], parity p = 2 py + px of the output pixel (2y + py, 2x + px), tap
// t = 2 ty + tx over the low-resolution pixel (y - 1 + py + ty, x - 1 + px + tx).  Along each axis the three taps fold as
//   parity 0: tap 0 = w[0], tap 1 = w[1] + w[2]          parity 1: tap 0 = w[0] + w[1], tap 1 = w[2]
// (the upsampled rows 2y - 1 | 2y, 2y + 1 are the low-resolution rows y - 1 | y, y, and 2y, 2y + 1 | 2y + 2 are y, y | y + 1); the
// up-to-four products are summed in float64 and rounded once.
extern "C" long ofx_upconv2x_weight(const float* w, int Cout, int Cin, float* out) {
    if (Cout <= 0 || Cin <= 0) return OFX_EINVAL;
    const long n = 16L * Cout * Cin;
    if (!out) return n;
    if (!w) return OFX_EINVAL;
    // fold[parity][tap][k]: does 3-tap index k belong to folded tap `tap`
    static const int fold[2][2][3] = {{{1, 0, 0}, {0, 1, 1}}, {{1, 1, 0}, {0, 0, 1}}};
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px)
            for (int o = 0; o < Cout; ++o)
                for (int ty = 0; ty < 2; ++ty)
                    for (int tx = 0; tx < 2; ++tx)
                        for (int c = 0; c < Cin; ++c) {
                            const float* g = w + ((size_t)o * Cin + c) * 9;
                            double s = 0.0;
                            for (int ky = 0; ky < 3; ++ky)
                                for (int kx = 0; kx < 3; ++kx)
                                    if (fold[py][ty][ky] && fold[px][tx][kx]) s += (double)g[ky * 3 + kx];
                            out[((((size_t)(2 * py + px) * Cout + o) * 4 + 2 * ty + tx)) * Cin + c] = (float)s;
                        }
    return n;
}

extern "C" int ofx_upconv2x_bn(int Cout, int precision) {
    if (Cout <= 0 || (precision != OFX_PREC_FP32 && precision != OFX_PREC_F16 && precision != OFX_PREC_F16_W)) return OFX_EINVAL;
    return Cout <= 64 ? 64 : 128;
}

// the checks and the launch of both entry points; precision is OFX_PREC_FP32, OFX_PREC_F16 or OFX_PREC_F16_W (w: halves) here
static int upconv2x_checked(const float* x, const float* w, const float* bias, float* out, int ldo, int B, int H, int W, int Cin,
                            int Cout, int precision, void* stream) {
    OFX_REQUIRE(x && w && out, OFX_EINVAL);
    OFX_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && ldo >= Cout, OFX_EINVAL);
    OFX_REQUIRE(Cin % 4 == 0 && ofx_aligned16(x) && ofx_aligned16(w), OFX_EALIGN);
    OFX_REQUIRE((((uintptr_t)out) & 3u) == 0 && (!bias || (((uintptr_t)bias) & 3u) == 0), OFX_EALIGN);
    // rows and pixels are 32-bit ints in the kernel (addresses are 64-bit): the upsampled map must have fewer than 2^31 pixels
    const long M = (long)B * H * W;
    OFX_REQUIRE(4 * M < (1L << 31), OFX_EINVAL);
    UpK k;
    k.x = x; k.w = w; k.bias = bias; k.out = out;
    k.B = B; k.H = H; k.W = W; k.Cin = Cin; k.Cout = Cout; k.ldo = ldo;
    k.M = (int)M;
    const bool f16w = precision == OFX_PREC_F16_W, f16 = precision == OFX_PREC_F16 || f16w;
    const int bk = f16 ? kBKh : kBK;
    k.cchunks = (Cin + bk - 1) / bk;
    const int bn = ofx_upconv2x_bn(Cout, precision);
    k.ntiles = (Cout + bn - 1) / bn;
    const long mtiles = (M + 127) / 128;
    OFX_REQUIRE(mtiles * k.ntiles < (1L << 31), OFX_EINVAL);
    hipStream_t s = (hipStream_t)stream;
    OfxProfScope prof(f16 ? "upconv2x_f16" : "upconv2x", s);
    prof.flops(2.0 * 4.0 * (double)M * Cout * 4.0 * Cin);
    dim3 grid((unsigned)(mtiles * k.ntiles), 4, 1), block(256, 1, 1);
    if (f16w) {
        if (bn == 64) hipLaunchKernelGGL((upconv2x_kernel<64, OFX_PREC_F16_W>), grid, block, 0, s, k);
        else hipLaunchKernelGGL((upconv2x_kernel<128, OFX_PREC_F16_W>), grid, block, 0, s, k);
    } else if (f16) {
        if (bn == 64) hipLaunchKernelGGL((upconv2x_kernel<64, OFX_PREC_F16>), grid, block, 0, s, k);
        else hipLaunchKernelGGL((upconv2x_kernel<128, OFX_PREC_F16>), grid, block, 0, s, k);
    } else {
        if (bn == 64) hipLaunchKernelGGL(upconv2x_kernel<64>, grid, block, 0, s, k);
        else hipLaunchKernelGGL(upconv2x_kernel<128>, grid, block, 0, s, k);
    }
    return ofx_launch_status();
}

extern "C" int ofx_upconv2x(const float* x, const float* w, const float* bias, float* out, int ldo, int B, int H, int W, int Cin,
                            int Cout, void* stream) {
    return upconv2x_checked(x, w, bias, out, ldo, B, H, W, Cin, Cout, OFX_PREC_FP32, stream);
}

extern "C" int ofx_upconv2x_prec(const float* x, const float* w, const float* bias, float* out, int ldo, int B, int H, int W, int Cin,
                                 int Cout, int precision, void* stream) {
    OFX_REQUIRE(precision == OFX_PREC_FP32 || precision == OFX_PREC_F16 || precision == OFX_PREC_F16_W, OFX_EINVAL);
    if (precision == OFX_PREC_FP32) return ofx_upconv2x(x, w, bias, out, ldo, B, H, W, Cin, Cout, stream);
    return upconv2x_checked(x, w, bias, out, ldo, B, H, W, Cin, Cout, precision, stream);
}

extern "C" int ofx_upsample2x_nearest_f32(const float* in, float* out, int B, int H, int W, int C, void* stream) {
    OFX_REQUIRE(in && out && B > 0 && H > 0 && W > 0 && C > 0, OFX_EINVAL);
    OFX_REQUIRE(C % 4 == 0 && ofx_aligned16(in) && ofx_aligned16(out), OFX_EALIGN);
    OFX_REQUIRE(4L * B * H * W < (1L << 31), OFX_EINVAL);
    const size_t total = (size_t)4 * B * H * W * (C / 4);
    hipStream_t s = (hipStream_t)stream;
    OfxProfScope prof("upsample2x_nearest", s);
    const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(upsample2x_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const float4*>(in), reinterpret_cast<float4*>(out),
                       H, W, C / 4, total);
    return ofx_launch_status();
}

extern "C" int ofx_decode_to_u8(const float* x, int ld, uint8_t* out, int B, int H, int W, void* stream) {
    OFX_REQUIRE(x && out && B > 0 && H > 0 && W > 0 && ld >= 3, OFX_EINVAL);
    OFX_REQUIRE((((uintptr_t)x) & 3u) == 0 && (((uintptr_t)out) & 3u) == 0, OFX_EALIGN);
    const size_t npix = (size_t)B * H * W;
    OFX_REQUIRE(npix < ((size_t)1 << 33), OFX_EINVAL);       // one thread per four pixels, at most 2^31 - 1 workgroups
    hipStream_t s = (hipStream_t)stream;
    OfxProfScope prof("decode_to_u8", s);
    const size_t groups = (npix + 3) / 4;
    hipLaunchKernelGGL(decode_to_u8_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, s, x, ld, out, npix);
    return ofx_launch_status();
}
