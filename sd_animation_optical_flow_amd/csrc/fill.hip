// fill_mask_input (guided_ldm_inpainting.py:161-176), what img2img_inpaint does to its frame when it has no reference (:295-296):
// the masked region is filled with colours bled in from its surroundings by a cascade of Gaussian blurs, all in Pillow's 8-bit
// integer arithmetic and bit-exact to it:
//
//   pasted = paste(image as premultiplied RGBa, mask = 255 - image_mask) onto zeros         Paste.c    p = DIV255(c * inv), a = inv
//   for (radius, repeats) in (256,1) (64,1) (16,2) (4,4) (2,2) (0,1):
//       layer = GaussianBlur(radius)(pasted).convert('RGBA')                                BoxBlur.c, Convert.c rgba2rgbA
//       accumulator.alpha_composite(layer), `repeats` times                                 AlphaComposite.c
//   out = accumulator.convert('RGB')
//
// The hot part is the blur of a 4-channel image at box radius up to 255.  box_blur_rows_kernel (handoff.hip) adds its 2r+1 taps
// per pixel, fine for the mask's r = 3; here a row is prefix-summed in LDS instead and every output is a difference of two prefix
// entries plus the replicated-edge terms, so a pass costs the same at every radius.  Between the axes the image is transposed, as
// in the single-channel blur (ofx_transpose_tile_kernel, 4-byte pixels).
#include "ofx_internal.h"

#include <algorithm>

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// LDS per row of W pixels: the prefix sums (4 x uint32 = 16 B per pixel) and two copies of the packed row (4 B each) = 24 W bytes.
// 6144 pixels are 144 KiB of the CU's 160 KiB (plus the 64 B of wave totals).
constexpr int kBlurMaxSide = 6144;
constexpr int kBlurLdsPerPixel = 24;

__device__ __forceinline__ u32x4 unpack4(unsigned p) { return u32x4{p & 255u, (p >> 8) & 255u, (p >> 16) & 255u, p >> 24}; }
__device__ __forceinline__ unsigned pack4(u32x4 v) { return v.x | (v.y << 8) | (v.z << 16) | (v.w << 24); }

// One workgroup per row of an interleaved 4 x 8-bit image; `passes` extended-box passes (ImagingLineBoxBlur32: replicated edges,
// out = (acc*ww + (left_far + right_far)*fw + 2^23) >> 24 in uint32, the four channels alike).  Per pass:
//   1. thread t sums its K consecutive pixels; the totals are scanned across the wave (__shfl_up) and the four wave totals go
//      through LDS, which gives every thread the prefix in front of its chunk
//   2. the thread walks its chunk again and writes the inclusive prefix S[x] (16 B per pixel)
//   3. every output: acc = S[min(x+r, W-1)] - S[x-r-1] + a[0] * max(0, r-x) + a[W-1] * max(0, x+r-(W-1))
// K is odd, so the chunk walks of a wave hit distinct banks: lane stride K dwords for the 4-byte reads, 4K dwords for the 16-byte
// writes (8 consecutive lanes cover 4K * {0..7} mod 32 = all eight 4-bank slots).  Step 3 reads consecutive 16-byte slots.
__global__ __launch_bounds__(256) void box_blur_rows_rgba_kernel(const uint32_t* in, uint32_t* out, int W, int K,   // in == out is allowed
                                                                 int r, unsigned ww, unsigned fw, int passes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fill_smem[];
    __shared__ u32x4 wave_tot[4];
    u32x4* S = reinterpret_cast<u32x4*>(fill_smem);
    uint32_t* a = reinterpret_cast<uint32_t*>(fill_smem + (size_t)16 * W);
    uint32_t* b = a + W;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long base = (long)blockIdx.x * W;
    for (int x = t; x < W; x += 256) a[x] = in[base + x];
    __syncthreads();
    const int x0 = min(t * K, W), x1 = min(x0 + K, W);
    for (int p = 0; p < passes; ++p) {
        u32x4 tot = {0u, 0u, 0u, 0u};
        for (int x = x0; x < x1; ++x) tot += unpack4(a[x]);
        u32x4 inc = tot;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            u32x4 o;
            o.x = __shfl_up(inc.x, d);
            o.y = __shfl_up(inc.y, d);
            o.z = __shfl_up(inc.z, d);
            o.w = __shfl_up(inc.w, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wave_tot[wave] = inc;
        __syncthreads();
        u32x4 run = inc - tot;
        for (int w = 0; w < wave; ++w) run += wave_tot[w];
        for (int x = x0; x < x1; ++x) {
            run += unpack4(a[x]);
            S[x] = run;
        }
        __syncthreads();
        const u32x4 first = unpack4(a[0]), last = unpack4(a[W - 1]);
        for (int x = t; x < W; x += 256) {
            const int hi = min(x + r, W - 1), lo = x - r - 1;
            u32x4 acc = S[hi];
            if (lo >= 0) acc -= S[lo];
            acc += first * (unsigned)max(0, r - x) + last * (unsigned)max(0, x + r - (W - 1));
            const u32x4 far_ = unpack4(a[max(lo, 0)]) + unpack4(a[min(x + r + 1, W - 1)]);
            const u32x4 bulk = acc * ww + far_ * fw;
            b[x] = pack4((bulk + (1u << 23)) >> 24);
        }
        __syncthreads();
        uint32_t* s = a; a = b; b = s;
    }
    for (int x = t; x < W; x += 256) out[base + x] = a[x];
}

__device__ __forceinline__ unsigned shift255(unsigned a) { return (a + (a >> 8)) >> 8; }   // AlphaComposite.c SHIFTFORDIV255

// the opaque frame pasted onto an empty premultiplied canvas through 255 - mask
__global__ __launch_bounds__(256) void fill_paste_kernel(const uint8_t* __restrict__ image, const uint8_t* __restrict__ mask,
                                                         uint32_t* __restrict__ pasted, long total) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const unsigned inv = 255u - mask[i];
        u32x4 v;
        v.x = ofx_div255(image[i * 3 + 0] * inv);
        v.y = ofx_div255(image[i * 3 + 1] * inv);
        v.z = ofx_div255(image[i * 3 + 2] * inv);
        v.w = ofx_div255(255u * inv);
        pasted[i] = pack4(v);
    }
}

// One stage of the cascade behind its blur: 'RGBa' -> 'RGBA' of the blurred pixel, then `repeats` alpha_composites of it onto the
// accumulator (`first`: the accumulator starts empty and is not read).  The last stage writes the three colours to out_rgb
// (convert('RGB')) instead of the accumulator.
__global__ __launch_bounds__(256) void fill_stage_kernel(const uint32_t* __restrict__ blurred, uint32_t* __restrict__ accum,
                                                         uint8_t* __restrict__ out_rgb, int repeats, int first, long total) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        u32x4 s = unpack4(blurred[i]);
        if (s.w != 0u && s.w != 255u) {
            s.x = min(255u, 255u * s.x / s.w);
            s.y = min(255u, 255u * s.y / s.w);
            s.z = min(255u, 255u * s.z / s.w);
        }
        u32x4 d = first ? u32x4{0u, 0u, 0u, 0u} : unpack4(accum[i]);
        if (s.w != 0u) {
            for (int k = 0; k < repeats; ++k) {
                const unsigned outa255 = s.w * 255u + d.w * (255u - s.w);
                const unsigned coef1 = s.w * 255u * 255u * 128u / outa255;
                const unsigned coef2 = 255u * 128u - coef1;
                d.x = shift255(s.x * coef1 + d.x * coef2 + (0x80u << 7)) >> 7;
                d.y = shift255(s.y * coef1 + d.y * coef2 + (0x80u << 7)) >> 7;
                d.z = shift255(s.z * coef1 + d.z * coef2 + (0x80u << 7)) >> 7;
                d.w = shift255(outa255 + 0x80u);
            }
        }
        if (out_rgb) {
            out_rgb[i * 3 + 0] = (uint8_t)d.x;
            out_rgb[i * 3 + 1] = (uint8_t)d.y;
            out_rgb[i * 3 + 2] = (uint8_t)d.z;
        } else {
            accum[i] = pack4(d);
        }
    }
}

int grid1d(long total) { return (int)std::min<long>((total + 255) / 256, 256L * 32); }

bool aligned4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

bool blur_args_ok(int B, int H, int W, float radius) {
    return B > 0 && B <= 65535 && H > 0 && W > 0 && std::max(H, W) <= kBlurMaxSide && radius >= 0.f && radius <= 65536.f;
}

// the four launches of one blur (radius > 0); arguments validated by the caller
int blur_rgba_launch(const uint32_t* in, uint32_t* out, uint32_t* scratch, int B, int H, int W, float radius, hipStream_t s) {
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&box_blur_rows_rgba_kernel),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, kBlurLdsPerPixel * kBlurMaxSide);
    OFX_HIP_CHECK(attr);
    int r;
    unsigned ww, fw;
    ofx_gaussian_box_weights(radius, 3, &r, &ww, &fw);
    const int KW = ofx_cdiv(W, 256) | 1, KH = ofx_cdiv(H, 256) | 1;
    hipLaunchKernelGGL(box_blur_rows_rgba_kernel, dim3((unsigned)((long)B * H)), dim3(256), (size_t)kBlurLdsPerPixel * W, s, in, out, W, KW, r,
                       ww, fw, 3);
    hipLaunchKernelGGL(ofx_transpose_tile_kernel<uint32_t>, dim3(ofx_cdiv(W, 32), ofx_cdiv(H, 32), B), dim3(256), 0, s, out, scratch, H, W);
    hipLaunchKernelGGL(box_blur_rows_rgba_kernel, dim3((unsigned)((long)B * W)), dim3(256), (size_t)kBlurLdsPerPixel * H, s, scratch, scratch,
                       H, KH, r, ww, fw, 3);
    hipLaunchKernelGGL(ofx_transpose_tile_kernel<uint32_t>, dim3(ofx_cdiv(H, 32), ofx_cdiv(W, 32), B), dim3(256), 0, s, scratch, out, W, H);
    return ofx_launch_status();
}

size_t plane_bytes(int B, int H, int W) { return (((size_t)B * H * W * 4) + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int ofx_gaussian_blur_rgba_u8(const uint8_t* in, uint8_t* out, uint8_t* scratch, int B, int H, int W, float radius, void* stream) {
    OFX_REQUIRE(in && out && aligned4(in) && aligned4(out), OFX_EINVAL);
    OFX_REQUIRE(blur_args_ok(B, H, W, radius), OFX_EINVAL);
    hipStream_t s = (hipStream_t)stream;
    if (radius == 0.f) {
        if (in != out) OFX_HIP_CHECK(hipMemcpyAsync(out, in, (size_t)B * H * W * 4, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    OFX_REQUIRE(scratch && aligned4(scratch) && scratch != in && scratch != out, OFX_EINVAL);
    OfxProfScope prof("gaussian_blur_rgba_u8", s);
    return blur_rgba_launch(reinterpret_cast<const uint32_t*>(in), reinterpret_cast<uint32_t*>(out), reinterpret_cast<uint32_t*>(scratch), B, H,
                            W, radius, s);
}

size_t ofx_fill_mask_input_scratch_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return 4 * plane_bytes(B, H, W);
}

int ofx_fill_mask_input(const uint8_t* image_bgr, const uint8_t* mask, uint8_t* out_bgr, void* scratch, int B, int H, int W, void* stream) {
    OFX_REQUIRE(image_bgr && mask && out_bgr && scratch && ofx_aligned16(scratch), OFX_EINVAL);
    OFX_REQUIRE(blur_args_ok(B, H, W, 0.f), OFX_EINVAL);
    OFX_REQUIRE(scratch != (const void*)image_bgr && scratch != (const void*)mask && scratch != (void*)out_bgr, OFX_EINVAL);
    hipStream_t s = (hipStream_t)stream;
    const size_t pb = plane_bytes(B, H, W);
    uint8_t* base = static_cast<uint8_t*>(scratch);
    uint32_t* pasted = reinterpret_cast<uint32_t*>(base);
    uint32_t* blurred = reinterpret_cast<uint32_t*>(base + pb);
    uint32_t* tmp = reinterpret_cast<uint32_t*>(base + 2 * pb);
    uint32_t* accum = reinterpret_cast<uint32_t*>(base + 3 * pb);
    const long total = (long)B * H * W;
    OfxProfScope prof("fill_mask_input", s);
    hipLaunchKernelGGL(fill_paste_kernel, dim3(grid1d(total)), dim3(256), 0, s, image_bgr, mask, pasted, total);
    static const struct { float radius; int repeats; } kStages[] = {{256.f, 1}, {64.f, 1}, {16.f, 2}, {4.f, 4}, {2.f, 2}, {0.f, 1}};
    const int n = (int)(sizeof(kStages) / sizeof(kStages[0]));
    for (int i = 0; i < n; ++i) {
        const uint32_t* layer = pasted;                       // GaussianBlur(0) is a copy
        if (kStages[i].radius > 0.f) {
            const int e = blur_rgba_launch(pasted, blurred, tmp, B, H, W, kStages[i].radius, s);
            if (e) return e;
            layer = blurred;
        }
        hipLaunchKernelGGL(fill_stage_kernel, dim3(grid1d(total)), dim3(256), 0, s, layer, accum, i == n - 1 ? out_bgr : (uint8_t*)nullptr,
                           kStages[i].repeats, i == 0 ? 1 : 0, total);
    }
    return ofx_launch_status();
}

}  // extern "C"
