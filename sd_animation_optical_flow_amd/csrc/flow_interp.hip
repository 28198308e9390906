// forward_interpolate of RAFT/core/utils/utils.py:26-53 on the device: the warm start of a video chain carries the previous pair's
// 1/8-resolution flow forward along itself.  Every grid pixel (x0, y0) of a field is a source at (x1, y1) = (x0 + dx, y0 + dy) in
// float64 (x0 + (double)dx is exact, as numpy's int64 + float32 -> float64); a source is valid iff 0 < x1 < w and 0 < y1 < h, both
// strict.  Every output pixel takes the (dx, dy) of the valid source nearest to its integer position -- scipy's
// griddata(method='nearest'), a cKDTree query on the squared Euclidean distance (x1 - x0)^2 + (y1 - y0)^2 in float64: two rounded
// products and one rounded add, never an FMA (this file is compiled with -ffp-contract=off and spells the roundings out too).
//
//   count   valid sources per unit cell (floor(x1), floor(y1)): every valid source lies inside the h x w grid, so h*w cells a field
//   scan    exclusive offsets of the cells
//   fill    source indices bucketed by cell (atomics: arbitrary order inside a cell)
//   search  per output pixel, cells in growing Chebyshev rings until no unvisited source can be nearer; the minimum of
//           (d2, source index) decides, so the result does not depend on the order the atomics left inside a cell
//
// Ties: the lowest source index among the sources at the smallest distance (scipy's choice among ties depends on its tree's shape).
// A field without any valid source gives NaN everywhere, as the reference does.  Fields are independent ([B, h, w, 2] in and out).
#include "ofx_internal.h"

#include <cmath>

namespace {

struct FiSource {
    double x1, y1;
    bool valid;
};

__device__ __forceinline__ FiSource fi_source(const float2 f, int x0, int y0, int h, int w) {
    FiSource s;
    s.x1 = __dadd_rn((double)x0, (double)f.x);
    s.y1 = __dadd_rn((double)y0, (double)f.y);
    s.valid = s.x1 > 0.0 && s.x1 < (double)w && s.y1 > 0.0 && s.y1 < (double)h;   // NaN compares false: never a source
    return s;
}

__device__ __forceinline__ int fi_cell(const FiSource& s, int w) { return (int)floor(s.y1) * w + (int)floor(s.x1); }

__global__ __launch_bounds__(256) void fi_count_kernel(const float* __restrict__ flow, int* __restrict__ cnt, int h, int w, long total) {
    const int N = h * w;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
        const long b = g / N;
        const int i = (int)(g - b * N), y0 = i / w, x0 = i - y0 * w;
        const FiSource s = fi_source(reinterpret_cast<const float2*>(flow)[g], x0, y0, h, w);
        if (s.valid) atomicAdd(cnt + b * N + fi_cell(s, w), 1);
    }
}

// one workgroup per field: exclusive scan of the N cell counts into off[0..N] (off[N] = valid sources of the field).  Each of the 1024
// threads takes 8 consecutive cells per pass; wavefront scans with cross-lane shifts, then the 16 wavefront totals.
constexpr int kScanThreads = 1024, kScanPer = 8;

__global__ __launch_bounds__(kScanThreads) void fi_scan_kernel(const int* __restrict__ cnt, int* __restrict__ off, int N) {
    const int* c = cnt + (long)blockIdx.x * N;
    int* o = off + (long)blockIdx.x * (N + 1);
    __shared__ int wsum[kScanThreads / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < N; base += kScanThreads * kScanPer) {
        const int i0 = base + threadIdx.x * kScanPer;
        int v[kScanPer], s = 0;
#pragma unroll
        for (int k = 0; k < kScanPer; ++k) {
            v[k] = i0 + k < N ? c[i0 + k] : 0;
            s += v[k];
        }
        int x = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        if (wv == 0) {
            int t = lane < kScanThreads / 64 ? wsum[lane] : 0;
#pragma unroll
            for (int d = 1; d < kScanThreads / 64; d <<= 1) {
                const int y = __shfl_up(t, d, 64);
                if (lane >= d) t += y;
            }
            if (lane < kScanThreads / 64) wsum[lane] = t;
        }
        __syncthreads();
        int e = carry + (wv ? wsum[wv - 1] : 0) + x - s;
#pragma unroll
        for (int k = 0; k < kScanPer; ++k) {
            if (i0 + k < N) o[i0 + k] = e;
            e += v[k];
        }
        carry += wsum[kScanThreads / 64 - 1];
        __syncthreads();   // wsum is rewritten by the next pass
    }
    if (threadIdx.x == 0) o[N] = carry;
}

// cnt counts down to zero while the slots of each cell are handed out
__global__ __launch_bounds__(256) void fi_fill_kernel(const float* __restrict__ flow, int* __restrict__ cnt, const int* __restrict__ off,
                                                      int* __restrict__ idx, int h, int w, long total) {
    const int N = h * w;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
        const long b = g / N;
        const int i = (int)(g - b * N), y0 = i / w, x0 = i - y0 * w;
        const FiSource s = fi_source(reinterpret_cast<const float2*>(flow)[g], x0, y0, h, w);
        if (!s.valid) continue;
        const int c = fi_cell(s, w);
        const int slot = atomicSub(cnt + b * N + c, 1) - 1;
        idx[b * N + off[b * (N + 1) + c] + slot] = i;
    }
}

struct FiBest {
    double d2;
    int i;
};

__device__ __forceinline__ void fi_visit(const float2* __restrict__ fl, const int* __restrict__ off, const int* __restrict__ idx, int cx,
                                         int cy, int px, int py, int h, int w, FiBest& best) {
    if ((unsigned)cx >= (unsigned)w || (unsigned)cy >= (unsigned)h) return;
    const int c = cy * w + cx;
    for (int k = off[c], e = off[c + 1]; k < e; ++k) {
        const int i = idx[k];
        const int y0 = i / w, x0 = i - y0 * w;
        const FiSource s = fi_source(fl[i], x0, y0, h, w);
        const double dx = __dsub_rn(s.x1, (double)px), dy = __dsub_rn(s.y1, (double)py);
        const double d2 = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
        if (d2 < best.d2 || (d2 == best.d2 && i < best.i)) {
            best.d2 = d2;
            best.i = i;
        }
    }
}

// Ring R around pixel (px, py) = the cells whose per-axis cell distance (cx - px for cx >= px, px - 1 - cx below) peaks at R: the
// border of [px-1-R, px+R] x [py-1-R, py+R].  A source in such a cell is at least R away on one axis, so once rings 0..R are visited
// every other source has d2 >= (R+1)^2 -- also after rounding, which is monotonic -- and the search stops when best.d2 < (R+1)^2.
__global__ __launch_bounds__(256) void fi_search_kernel(const float* __restrict__ flow, const int* __restrict__ off,
                                                        const int* __restrict__ idx, float* __restrict__ out, int h, int w, long total) {
    const int N = h * w;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
        const long b = g / N;
        const int p = (int)(g - b * N), py = p / w, px = p - py * w;
        const float2* fl = reinterpret_cast<const float2*>(flow) + b * N;
        const int* of = off + b * (N + 1);
        const int* ix = idx + b * N;
        if (of[N] == 0) {   // no valid source in this field
            reinterpret_cast<float2*>(out)[g] = make_float2(NAN, NAN);
            continue;
        }
        FiBest best{INFINITY, 0x7fffffff};
        for (int R = 0;; ++R) {
            const int xl = px - 1 - R, xh = px + R, yl = py - 1 - R, yh = py + R;
            for (int cx = max(xl, 0); cx <= min(xh, w - 1); ++cx) {
                fi_visit(fl, of, ix, cx, yl, px, py, h, w, best);
                fi_visit(fl, of, ix, cx, yh, px, py, h, w, best);
            }
            for (int cy = max(yl + 1, 0); cy <= min(yh - 1, h - 1); ++cy) {
                fi_visit(fl, of, ix, xl, cy, px, py, h, w, best);
                fi_visit(fl, of, ix, xh, cy, px, py, h, w, best);
            }
            const double next = (double)(R + 1) * (double)(R + 1);
            if (best.d2 < next) break;
            if (xl <= 0 && yl <= 0 && xh >= w - 1 && yh >= h - 1) break;   // every cell visited
        }
        reinterpret_cast<float2*>(out)[g] = fl[best.i];
    }
}

static inline unsigned fi_blocks(long n) { return (unsigned)std::max<long>(1, std::min<long>((n + 255) / 256, 16384)); }

}  // namespace

extern "C" {

size_t ofx_forward_interpolate_scratch_bytes(int B, int h, int w) {
    if (B <= 0 || h <= 0 || w <= 0 || (long)h * w >= (1L << 30)) return 0;
    const long N = (long)h * w;
    return (size_t)B * (size_t)(3 * N + 1) * sizeof(int);   // off [B][N+1] | cnt [B][N] | idx [B][N]
}

int ofx_forward_interpolate(const float* flow, float* out, void* scratch, size_t scratch_bytes, int B, int h, int w, void* stream) {
    OFX_REQUIRE(flow && out && scratch && B > 0 && h > 0 && w > 0 && flow != out, OFX_EINVAL);
    const size_t need = ofx_forward_interpolate_scratch_bytes(B, h, w);
    OFX_REQUIRE(need > 0 && scratch_bytes >= need, OFX_EINVAL);
    OFX_REQUIRE((((uintptr_t)flow) & 7u) == 0 && (((uintptr_t)out) & 7u) == 0 && (((uintptr_t)scratch) & 3u) == 0, OFX_EALIGN);
    hipStream_t s = (hipStream_t)stream;
    const int N = h * w;
    const long total = (long)B * N;
    int* off = static_cast<int*>(scratch);
    int* cnt = off + (long)B * (N + 1);
    int* idx = cnt + total;
    OfxProfScope prof("forward_interpolate", s);
    OFX_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)total * sizeof(int), s));
    hipLaunchKernelGGL(fi_count_kernel, dim3(fi_blocks(total)), dim3(256), 0, s, flow, cnt, h, w, total);
    int st = ofx_launch_status();
    if (st) return st;
    for (long b0 = 0; b0 < B; b0 += 65535) {   // (one workgroup per field)
        const long nb = std::min<long>(65535, B - b0);
        hipLaunchKernelGGL(fi_scan_kernel, dim3((unsigned)nb), dim3(kScanThreads), 0, s, cnt + b0 * N, off + b0 * (N + 1), N);
        if ((st = ofx_launch_status())) return st;
    }
    hipLaunchKernelGGL(fi_fill_kernel, dim3(fi_blocks(total)), dim3(256), 0, s, flow, cnt, off, idx, h, w, total);
    if ((st = ofx_launch_status())) return st;
    hipLaunchKernelGGL(fi_search_kernel, dim3(fi_blocks(total)), dim3(256), 0, s, flow, off, idx, out, h, w, total);
    return ofx_launch_status();
}

}  // extern "C"
