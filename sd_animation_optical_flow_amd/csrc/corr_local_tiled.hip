// Volume-free local correlation, tiled through LDS (the engine's alternate_corr lookup; RAFT/core/corr.py:63-91 semantics).
//
// One workgroup (256 threads) owns an 8x8 tile of 1/8-grid pixels of one pair at one pyramid level.  The (2r+2)^2 tap windows of
// its 64 pixels overlap almost entirely when the flow is coherent, so the workgroup takes their bounding box in that level's
// fmap2, stages the box into LDS once per 16-channel slab (coalesced 16-byte loads) and every pixel forms its tap dot products
// from there.  local_corr_kernel (corr.hip) fetches each of a pixel's taps as a 1 KB row from L2 by itself: ~100 KB per pixel and
// level where this kernel fetches the box, ~5 KB per pixel at level 0.
//
//   lanes      lane = pixel of the tile (8 x 8, x fastest); the four waves split a pixel's taps: wave q owns taps q, q + 4, ...
//              ((2r+2)^2 / 4 = 25 accumulators at r = 4, 16 at r = 3, all in registers for the whole channel loop)
//   LDS        box rows at a fixed pitch of 24 positions, 20 floats per position (16 channels + one pad quad): with the pitch
//              = 8 mod 16 and the odd quad stride the 16 lanes that one ds_read_b128 group serves (two half rows of the tile and two
//              more, MI355X LDS banking) hit 16 different quad banks when neighbouring pixels read neighbouring positions.
//              One extra all-zero position serves every tap that falls outside the map, so the inner loop has no branch.
//   products   VALU from LDS: one ds_read_b128 feeds four FMAs; fmap1's 16 channels of the slab sit in registers
//   fallback   a tile whose box is wider or taller than 24 positions (incoherent flow) forms the same products straight from
//              global memory, tap by tap -- slow, correct, and the same accumulation order per tap
//   splat      the dot products go to LDS (over the slab), then the bilinear splat into the (2r+1)^2 outputs, x-major, in the
//              accumulation order of local_corr_kernel; output goes straight into the lookup rows (ld floats per pixel,
//              columns [level * (2r+1)^2, (level + 1) * (2r+1)^2)); other columns are never touched
//
// No atomics and no dependence on scheduling: every output is written once, by one thread, from a fixed summation order.
#include "ofx_internal.h"

namespace {

constexpr int kTile = 8;                 // pixels per tile side
constexpr int kPitch = 24;               // box positions per LDS row (= 8 mod 16) and the most box rows
constexpr int kSlab = 16;                // channels per slab
constexpr int kPosQuads = kSlab / 4 + 1; // float4 per position: 4 of data + 1 pad
constexpr int kZeroPos = kPitch * kPitch;
constexpr int kMaxLevels = 4;

struct TiledArgs {
    const float* f1;               // [n1][H1][W1][C]
    const float* f2[kMaxLevels];   // level l: [n2][H1 >> l][W1 >> l][C]
    const int* idx1;               // image of fmap1 per pair, or null: pair b uses image b
    const int* idx2;               // likewise for fmap2
    const float* coords;           // [B][H1][W1][2]
    float* out;                    // [B][H1][W1][ld]
    int ld, H1, W1, C, tiles_x;
    float scale;
};

template <int R>
__global__ __launch_bounds__(256) void local_corr_tiled_kernel(const TiledArgs a) {
    constexpr int WN = 2 * R + 2, RD = 2 * R + 1, NTAP = WN * WN, NT = NTAP / 4, DOTS_LD = NTAP + 1;
    static_assert(NTAP % 4 == 0, "the four waves split the taps evenly");
    static_assert((kZeroPos + 1) * kPosQuads * 4 >= kTile * kTile * DOTS_LD, "the dot products reuse the slab");
    __shared__ float4 slab[(kZeroPos + 1) * kPosQuads];
    __shared__ float sdx[kTile * kTile], sdy[kTile * kTile];

    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    const int level = blockIdx.y, b = blockIdx.z;
    const int H2 = a.H1 >> level, W2 = a.W1 >> level;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int px = tx * kTile + (lane & 7), py = ty * kTile + (lane >> 3);
    const bool live = px < a.W1 && py < a.H1;
    const long hw1 = (long)a.H1 * a.W1;
    const long pix = live ? (long)b * hw1 + (long)py * a.W1 + px : 0;
    const long i1 = a.idx1 ? a.idx1[b] : b, i2 = a.idx2 ? a.idx2[b] : b;
    const float* f1 = a.f1 + (i1 * hw1 + (live ? (long)py * a.W1 + px : 0)) * a.C;
    const float* f2 = a.f2[level] + i2 * (long)H2 * W2 * a.C;

    float x = 0.f, y = 0.f;
    if (live) {
        const float cscale = 1.0f / (float)(1 << level);
        const float2 c = reinterpret_cast<const float2*>(a.coords)[pix];
        x = c.x * cscale;
        y = c.y * cscale;
    }
    const bool sane = fabsf(x) < 1.0e7f && fabsf(y) < 1.0e7f;   // (NaN compares false)
    const int x0 = sane ? (int)floorf(x) : -100000, y0 = sane ? (int)floorf(y) : -100000;
    if (q == 0) {
        sdx[lane] = sane ? x - floorf(x) : 0.f;
        sdy[lane] = sane ? y - floorf(y) : 0.f;
    }

    // bounding box of the tile's windows, clipped to the map (every wave holds all 64 pixels: no exchange between waves)
    int bx0 = max(x0 - R, 0), bx1 = min(x0 + R + 1, W2 - 1), by0 = max(y0 - R, 0), by1 = min(y0 + R + 1, H2 - 1);
    if (!live || bx0 > bx1 || by0 > by1) {
        bx0 = by0 = INT_MAX;
        bx1 = by1 = INT_MIN;
    }
    for (int m = 32; m >= 1; m >>= 1) {
        bx0 = min(bx0, __shfl_xor(bx0, m, 64));
        by0 = min(by0, __shfl_xor(by0, m, 64));
        bx1 = max(bx1, __shfl_xor(bx1, m, 64));
        by1 = max(by1, __shfl_xor(by1, m, 64));
    }
    const bool any = bx0 <= bx1;                                   // else: every tap of the tile is outside the map
    const int bw = any ? bx1 - bx0 + 1 : 0, bh = any ? by1 - by0 + 1 : 0;
    const bool fits = bw <= kPitch && bh <= kPitch;                 // uniform over the workgroup

    float acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = 0.f;

    if (fits) {
        int off[NT];   // LDS position (in float4) of tap q + 4 j; taps outside the map read the zero position
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int t = j * 4 + q, iy = t / WN, ix = t - iy * WN;
            const int yy = y0 - R + iy, xx = x0 - R + ix;
            const bool in = live && (unsigned)yy < (unsigned)H2 && (unsigned)xx < (unsigned)W2;
            off[j] = (in ? (yy - by0) * kPitch + (xx - bx0) : kZeroPos) * kPosQuads;
        }
        if (tid < kPosQuads) slab[kZeroPos * kPosQuads + tid] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int nstage = bw * bh * (kSlab / 4);
        for (int c0 = 0; c0 < a.C && any; c0 += kSlab) {
            __syncthreads();                                        // the previous slab has been consumed
            for (int i = tid; i < nstage; i += 256) {
                const int p = i >> 2, cq = i & 3;
                const int ry = p / bw, rx = p - ry * bw;
                slab[(ry * kPitch + rx) * kPosQuads + cq] =
                    *reinterpret_cast<const float4*>(f2 + ((long)(by0 + ry) * W2 + bx0 + rx) * a.C + c0 + cq * 4);
            }
            float4 u[kSlab / 4];
#pragma unroll
            for (int cq = 0; cq < kSlab / 4; ++cq)
                u[cq] = live ? *reinterpret_cast<const float4*>(f1 + c0 + cq * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                float s = acc[j];
#pragma unroll
                for (int cq = 0; cq < kSlab / 4; ++cq) {
                    const float4 v = slab[off[j] + cq];
                    s = fmaf(u[cq].x, v.x, s);
                    s = fmaf(u[cq].y, v.y, s);
                    s = fmaf(u[cq].z, v.z, s);
                    s = fmaf(u[cq].w, v.w, s);
                }
                acc[j] = s;
            }
        }
    } else if (live) {
        // the box does not fit: this pixel's taps straight from global memory, channels in the same order
#pragma unroll 1
        for (int j = 0; j < NT; ++j) {
            const int t = j * 4 + q, iy = t / WN, ix = t - iy * WN;
            const int yy = y0 - R + iy, xx = x0 - R + ix;
            if ((unsigned)yy >= (unsigned)H2 || (unsigned)xx >= (unsigned)W2) continue;
            const float* g = f2 + ((long)yy * W2 + xx) * a.C;
            float s = 0.f;
            for (int c = 0; c < a.C; c += 4) {
                const float4 u = *reinterpret_cast<const float4*>(f1 + c);
                const float4 v = *reinterpret_cast<const float4*>(g + c);
                s = fmaf(u.x, v.x, s);
                s = fmaf(u.y, v.y, s);
                s = fmaf(u.z, v.z, s);
                s = fmaf(u.w, v.w, s);
            }
            acc[j] = s;
        }
    }

    __syncthreads();                                                // every wave is done with the slab
    float* dots = reinterpret_cast<float*>(slab);
#pragma unroll
    for (int j = 0; j < NT; ++j) dots[lane * DOTS_LD + j * 4 + q] = acc[j];
    __syncthreads();

    // bilinear splat (correlation_kernel.cu:92-114 semantics, local_corr_kernel's order of contributions)
    for (int i = tid; i < kTile * kTile * RD * RD; i += 256) {
        const int p = i / (RD * RD), k = i - p * (RD * RD);
        const int ox = tx * kTile + (p & 7), oy = ty * kTile + (p >> 3);
        if (ox >= a.W1 || oy >= a.H1) continue;
        const int kx = k / RD, ky = k - kx * RD;                   // channel = ky + RD * kx
        const float dx = sdx[p], dy = sdy[p];
        const float* s = dots + p * DOTS_LD;
        float v = s[ky * WN + kx] * (1.f - dy) * (1.f - dx);
        v += s[ky * WN + kx + 1] * (1.f - dy) * dx;
        v += s[(ky + 1) * WN + kx] * dy * (1.f - dx);
        v += s[(ky + 1) * WN + kx + 1] * dy * dx;
        a.out[((long)b * hw1 + (long)oy * a.W1 + ox) * a.ld + level * (RD * RD) + k] = v * a.scale;
    }
}

}  // namespace

// all `levels` pyramid levels of B pairs in one launch; level l reads f2l[l] = [n2][h >> l][w >> l][C] and writes columns
// [l * (2r+1)^2, (l+1) * (2r+1)^2) of the ld-float rows of `out`.  C % 16 == 0, r = 3 or 4.
int ofx_local_corr_tiled_launch(const float* f1, const float* const* f2l, const int* idx1, const int* idx2, const float* coords, float* out,
                                int ld, int B, int h, int w, int C, int r, int levels, float scale, hipStream_t s) {
    OFX_REQUIRE(f1 && f2l && coords && out, OFX_EINVAL);
    OFX_REQUIRE(B > 0 && B <= 65535 && h > 0 && w > 0 && C > 0 && C % kSlab == 0, OFX_EINVAL);
    OFX_REQUIRE((r == 3 || r == 4) && levels >= 1 && levels <= kMaxLevels, OFX_EINVAL);
    OFX_REQUIRE((h >> (levels - 1)) >= 1 && (w >> (levels - 1)) >= 1, OFX_EINVAL);
    OFX_REQUIRE(ld >= levels * (2 * r + 1) * (2 * r + 1), OFX_EINVAL);
    OFX_REQUIRE(((((uintptr_t)f1) | ((uintptr_t)coords)) & 15u) == 0, OFX_EALIGN);
    TiledArgs a{};
    a.f1 = f1;
    for (int l = 0; l < levels; ++l) {
        OFX_REQUIRE(f2l[l] && (((uintptr_t)f2l[l]) & 15u) == 0, OFX_EALIGN);
        a.f2[l] = f2l[l];
    }
    a.idx1 = idx1; a.idx2 = idx2;
    a.coords = coords;
    a.out = out;
    a.ld = ld; a.H1 = h; a.W1 = w; a.C = C;
    a.tiles_x = (w + kTile - 1) / kTile;
    a.scale = scale;
    const long tiles = (long)a.tiles_x * ((h + kTile - 1) / kTile);
    OFX_REQUIRE(tiles < (1L << 31), OFX_EINVAL);
    const dim3 grid((unsigned)tiles, (unsigned)levels, (unsigned)B);
    OfxProfScope prof("local_corr_tiled", s);
    if (r == 4)
        hipLaunchKernelGGL(local_corr_tiled_kernel<4>, grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(local_corr_tiled_kernel<3>, grid, dim3(256), 0, s, a);
    return ofx_launch_status();
}

extern "C" int ofx_local_corr_rows(const float* fmap1, const float* const* fmap2_levels, const int* idx1, const int* idx2, const float* coords,
                                   float* rows, int ld, int B, int H1, int W1, int C, int levels, int radius, int tiled, void* stream) {
    OFX_REQUIRE(fmap1 && fmap2_levels && coords && rows, OFX_EINVAL);
    OFX_REQUIRE(B > 0 && H1 > 0 && W1 > 0 && C > 0 && levels >= 1 && levels <= kMaxLevels && radius >= 0, OFX_EINVAL);
    const float scale = 1.0f / sqrtf((float)C);
    if (tiled)
        return ofx_local_corr_tiled_launch(fmap1, fmap2_levels, idx1, idx2, coords, rows, ld, B, H1, W1, C, radius, levels, scale,
                                           (hipStream_t)stream);
    // the per-pixel kernel, launched as the engine launches it: one launch per level, image b for pair b
    OFX_REQUIRE(!idx1 && !idx2 && 2 * radius + 2 <= 10 && C % 4 == 0, OFX_EINVAL);
    const int rd2 = (2 * radius + 1) * (2 * radius + 1);
    OFX_REQUIRE(ld >= levels * rd2 && (H1 >> (levels - 1)) >= 1 && (W1 >> (levels - 1)) >= 1, OFX_EINVAL);
    for (int l = 0; l < levels; ++l) {
        OFX_REQUIRE(fmap2_levels[l], OFX_EINVAL);
        const int st = ofx_local_corr_launch(fmap1, fmap2_levels[l], coords, rows + (long)l * rd2, (long)H1 * W1 * ld, 0, 1, ld, B, H1, W1, H1 >> l,
                                             W1 >> l, C, 1, radius, scale, 1.0f / (float)(1 << l), (hipStream_t)stream);
        if (st) return st;
    }
    return 0;
}
