// Internal helpers shared by the HIP translation units of libofx.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/ofx.h"

#define OFX_HIP_CHECK(expr)                         \
    do {                                            \
        hipError_t _e = (expr);                     \
        if (_e != hipSuccess) return (int)_e;       \
    } while (0)

#define OFX_REQUIRE(cond, code) \
    do {                        \
        if (!(cond)) return (code); \
    } while (0)

static inline bool ofx_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
static inline int ofx_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---- profiling hooks (prof.cpp) -------------------------------------------------------
// Usage in a launcher:   OfxProfScope _p("kernel_name", stream);  kernel<<<...>>>(...);
// The scope records an event pair on `stream` when profiling is enabled and is free otherwise.
// ofx_prof_enable(2): launches are accumulated per "family:tag"; the RAFT executor tags each layer.
void ofx_prof_set_tag(const char* tag);   // thread-local; the pointer must outlive the launches it labels
struct OfxProfScope {
    int slot;
    hipStream_t stream;
    OfxProfScope(const char* name, hipStream_t s);
    ~OfxProfScope();
    void flops(double f);   // executed FLOPs of the bracketed launch (reported by ofx_prof_collect)
};

// Stop event of a launch (`ev`, may be null): the launcher hands it to hipExtLaunchKernelGGL as the kernel's own stop event, so
// the dependency edge to another stream rides on the dispatch packet's completion signal instead of a marker packet behind it
// (hipEventRecord): the caller's stream does not stall on the marker.  A launcher that takes a `stop_event` gives it to the LAST
// kernel it launches, so the event never fires before the call's work is done; a caller whose event was not taken (the call
// failed, or reports so through ConvExtra::stop_taken) records it the plain way.
#ifdef __HIPCC__
#include <hip/hip_ext.h>
#define OFX_LAUNCH(kern, grid, block, s, ev, ...)                                                  \
    do {                                                                                           \
        if (ev) {                                                                                  \
            hipExtLaunchKernelGGL(kern, grid, block, 0, s, nullptr, ev, 0, __VA_ARGS__);           \
        } else {                                                                                   \
            hipLaunchKernelGGL(kern, grid, block, 0, s, __VA_ARGS__);                              \
        }                                                                                          \
    } while (0)
#endif

static inline int ofx_launch_status() {
    hipError_t e = hipGetLastError();
    return (int)e;
}

// conv.hip: what a convolution call takes and gives besides its descriptor.  Everything is explicit: nothing travels between a
// caller and the launcher except through these fields.
struct ConvExtra {
    float alpha = 1.0f;              // extra scalar multiplier on the accumulator: out = act(acc * alpha * scale + shift)
    // the blocked correlation volume GEMM that also writes pyramid level 1 from its accumulators (out != null asks for it):
    // out = level 1, [nz][M][slice1] at zs floats per z; wb0 / wb1 = blocks per slice row of level 0 / 1
    struct Pool { float* out = nullptr; long zs = 0; int wb0 = 0, wb1 = 0, slice1 = 0; } pool;
    // instance-norm partial sums out of the epilogue (stats_rows != null asks for them): room for stats_cap floats in stats_part;
    // *stats_rows = rows per image written there, 0 = not produced
    float* stats_part = nullptr;
    size_t stats_cap = 0;
    int* stats_rows = nullptr;
    hipEvent_t stop_event = nullptr;   // rides on the last kernel launch of the call (see OFX_LAUNCH)
    bool* stop_taken = nullptr;        // optional out: a launch took stop_event (false: record it with hipEventRecord)
};
// The one entry of the convolution launcher; ofx_conv2d / ofx_conv2d_stats are ofx_conv2d_ex with the matching extras (null: none)
int ofx_conv2d_ex(const ofx_conv_desc* d, const ConvExtra* extra, hipStream_t s);
// ofx_conv_plan.path (ofx.h): the direct kernels, or a fused Winograd route of conv_wino.hip
enum { kPathIgemm = 0, kPathWino3x3 = 1, kPathWino15 = 2, kPathWino44 = 3, kPathWino44Fused = 4 };
// conv_wino.hip: the fused Winograd routes of ofx_conv2d -- F(4x4,3x3), F(2x2,3x3) and F(4,5), a table row each -- behind two
// entries.  The rule: which route takes a validated descriptor, given whether epilogue statistics are wanted (and the room for
// them, in floats), whether the pooled volume is, and the launcher's three switches (conv_knobs).  Pure: no HIP call, no
// environment, no global state.  Returns 0 with path = 0 (none: the direct kernels), or with the path, the rows per image of its
// statistics and the FLOPs it executes; OFX_EINVAL for a forced tile (OFX_CONV_TILE_WINOGRAD*) whose route does not take `d`.
struct OfxWinoChoice {
    int path = kPathIgemm, stats_rows = 0;
    double flops = 0.0;
};
int ofx_conv_wino_choose(const ofx_conv_desc* d, bool want_stats, size_t stats_cap, bool pool, bool no_wino, bool no_wino15, bool no_wino44,
                         OfxWinoChoice* c);
// ... and the launch of a chosen path (stats: null, or the room the choice was made with)
int ofx_conv_wino_launch(const ofx_conv_desc* d, int path, float alpha, float* stats, hipStream_t s, hipEvent_t stop_event);

// net_misc.hip: the per-image reduction of ofx_conv2d_stats' partials (ofx.h, ofx_inorm_finalize) with an optional
// gamma / beta (both or neither): an affine folded into the (mean, rstd) pair, (x - mean') * rstd' = (x - mu) * rs * gamma + beta
int ofx_inorm_finalize_part(const float* part, float* mean, float* rstd, int B, int rows, long HW, int C, float eps, hipStream_t s,
                            const float* gamma = nullptr, const float* beta = nullptr);
int ofx_inorm_stats_affine(const float* x, int ld, float* mean, float* rstd, float* scratch, int B, long HW, int C, float eps,
                           const float* gamma, const float* beta, hipStream_t stream);

// sd_ops.hip: the GroupNorm of ofx_groupnorm and ofx_groupnorm_cat (unet.hip), which validate -- nothing is checked here.  Carves
// `scratch` (ofx_groupnorm_scratch_bytes(B, C0 + C1)) into partial sums / scale / shift and launches partial -> finalize -> apply
// under the three profiler scope names.  One segment: x1 = null, C1 = 0; no per-image term: e = null (one dense segment without e
// runs the kernels' DENSE1 instantiation, whichever entry point asks)
int ofx_groupnorm_launch(const float* x0, int ld0, int C0, const float* x1, int ld1, int C1, const float* e, int lde, const float* gamma,
                         const float* beta, float* out, void* scratch, int B, long HW, int groups, float eps, int silu,
                         const char* const scope[3], hipStream_t s);

// attn_flash.hip: fused attention for the UNet's head sizes (no workspace).  precision: OFX_PREC_FP32 or OFX_PREC_F16 (the fp16
// matrix-core kernel, ofx_attention_prec); anything else is OFX_EINVAL before any launch
bool ofx_attention_flash_ok(int D);
int ofx_attention_flash_launch(const float* q, const float* k, const float* v, const float* bias, long bias_bstride, float* out, int BH, int Nq,
                               int Nk, int D, float scale, int precision, hipStream_t s);
// the same kernel on token rows with the heads side by side (ofx_attention_bnhd_f32, transformer.hip validates the arguments)
int ofx_attention_flash_bnhd_launch(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* bias,
                                    long bias_bstride, float* out, int ldo, int B, int H, int Nq, int Nk, int D, float scale, int precision,
                                    hipStream_t s);
// the strided kernels with K / V read through a segment table (ofx_attention_bnhd_segs, transformer.hip validates the arguments):
// image b owns the next counts[b] entries of `segs`, Nk is every image's total
int ofx_attention_flash_segs_launch(const float* q, int ldq, const ofx_kv_segment* segs, const int* counts, int kv_type, const float* bias,
                                    long bias_bstride, float* out, int ldo, int B, int H, int Nq, int Nk, int D, float scale, int precision,
                                    hipStream_t s);

// handoff.hip (compiled without FMA contraction): BoxBlur.c:_gaussian_blur_radius, the fractional box radius whose `passes`-fold
// application approximates GaussianBlur(radius), and ImagingHorizontalBoxBlur's weights from it: the integer radius r, the
// 2^24-scaled weight ww of a full tap and fw of the two fractional far taps.  Shared with fill.hip's 4-channel blur
float ofx_gaussian_box_radius(float radius, int passes);
void ofx_gaussian_box_weights(float radius, int passes, int* r, unsigned* ww, unsigned* fw);

// corr.hip / net_misc.hip: internal launchers used by the RAFT engine
int ofx_local_corr_launch(const float* f1, const float* f2, const float* coords, float* out, long sb, long sn,
                          long sc, long sp, int B, int H1, int W1, int H2, int W2, int C, int N, int r, float scale,
                          float cscale, hipStream_t s);
// corr_local_tiled.hip: the same lookup for all `levels` levels of B pairs in one launch, tap windows staged through LDS per 8x8 tile;
// f2l[l] = [n2][h >> l][w >> l][C] (host array of device pointers), idx1 / idx2 = device arrays of image indices per pair or null
// (pair b uses image b); writes columns [0, levels * (2r+1)^2) of the ld-float rows of `out`.  C % 16 == 0, r = 3 or 4
int ofx_local_corr_tiled_launch(const float* f1, const float* const* f2l, const int* idx1, const int* idx2, const float* coords, float* out,
                                int ld, int B, int h, int w, int C, int r, int levels, float scale, hipStream_t s);
// blocked pyramid layout (corr.hip): floats per pixel slice of an hl x wl level; fmap rows -> blocked order
int ofx_corr_slice_floats_l(int hl, int wl);
// ofx_corr_lookup that also writes `pad` (<= 47; 4 levels, radius 4 only) zeros behind the features of every output row
int ofx_corr_lookup_pad(const float* const* pyr, const float* coords, float* out, int ldo, int pad, int B, int h, int w, int levels,
                        int radius, void* stream);
int ofx_corr_block_rows(const float* src, float* dst, int n, int h, int w, int D, hipStream_t s);
int ofx_corr_pool_launch(const float* l0, float* l1, float* l2, float* l3, int B, int h, int w, int levels, hipStream_t s,
                         bool from_l1 = false);
bool ofx_corr_volpool_ok(int h, int w);
// corr_split.hip: the volume GEMM in split-bf16 form (opt-in `volume_precision`): fp32 rows -> bf16 planes in MFMA fragment order
// (planes = 2: bf16x3, 3: bf16x6; quad = 1: rows in the quad-blocked column order of the streamed operand), and the A-stationary GEMM
// that writes level 0 (blocked) and level 1 of nz pairs.  ia / ib: device arrays of image indices per pair, or null with byte strides
bool ofx_corr_volsplit_ok(int h, int w, int D);
bool ofx_corr_volsplit_pays(int nz, int h, int w, int planes);   // enough (pair, row group) tasks to fill the CUs' rounds
size_t ofx_corr_planes_bytes(int h, int w, int planes);
int ofx_corr_split_planes(const float* src, void* dst, int n, int h, int w, int planes, int quad, float alpha, hipStream_t s);
int ofx_corr_vol_split_launch(const void* ap, const void* bp, const int* ia, const int* ib, long a_zs, long b_zs, float* l0, float* l1,
                              int nz, int h, int w, int planes, hipStream_t s);
// mask_bits.hip: binary threshold/edge source -> elliptical dilation on bit planes
enum { OFX_MSRC_CONF_LT = 0, OFX_MSRC_CONF_NGT = 1, OFX_MSRC_EDGES = 3 };   // conf < t | !(conf > t) | Laplacian edges
int ofx_mask_bits_launch(int src, const float* conf, float* log_conf, const uint8_t* image, const uint8_t* or_mask,
                         uint8_t* out, int B, int H, int W, float thres, int edge_thres, int r, const signed char* hw,
                         const char* name, hipStream_t s);
// the route of that launch (host only; ofx_mask_plan of include/ofx.h with the element already made)
int ofx_mask_bits_plan(int src, int B, int H, int W, int r, const signed char* hw, int aligned16, ofx_mask_route* out);
// warp_fast.hip: bilinear warp of one shared uint8 RGB key frame (0 = launched, OFX_EINVAL = shape not taken)
int ofx_warp_bilinear_shared_launch(const uint8_t* frame, const float* flow, uint8_t* out, int B, int H, int W, float sign,
                                    hipStream_t s);
// warp_fast.hip: convex upsample + bilinear warp of one shared key frame in one pass (pad = zero-bordered RGBX copy of the frame)
size_t ofx_warp_pad_bytes(int H, int W);
bool ofx_upsample_warp_ok(int B, int H, int W);
int ofx_warp_pad_launch(const uint8_t* frame, void* pad, int H, int W, hipStream_t s);
int ofx_upsample_warp_launch(const float* coords1, const float* mask, float* flow_up, const void* pad, uint8_t* warped, int B, int h, int w,
                             float sign, hipStream_t s);
// warp_fast.hip: upflow8 (the small network's upsample) + bilinear warp of one shared key frame in one pass
int ofx_upflow8_warp_launch(const float* coords1, float* flow_up, const void* pad, uint8_t* warped, int B, int h, int w, float sign, hipStream_t s);
int ofx_init_state(float* coords1, float* frows, float* hx, int ldh, int flow_off, int B, int h, int w, hipStream_t s);
// ofx_init_state from an initial flow init f32 [B*h*w][2] (OFX_RAFT_FLOW_INIT): rows4 = the small network's [M][4] flow operand,
// else the basic network's 16-float convf1 rows
int ofx_init_state_warm(float* coords1, float* frows, float* hx, int ldh, int flow_off, bool rows4, const float* init, int B, int h,
                        int w, hipStream_t s);
int ofx_coords_to_flow(const float* coords1, float* flow, int B, int h, int w, hipStream_t s);
int ofx_flow_head_launch(const float* x, int ldx, const float* w, int Kpad, const float* bias, float* coords1, float* hx_flow,
                         int ldh, float* frows, int B, int h, int w_, hipStream_t s, hipEvent_t stop_event = nullptr);
int ofx_ctx_gather(const float* ctx, const int* idx_dev, float* hx, int ldh, int off2, int half, int B, long N, hipStream_t s);

// ---- device helpers --------------------------------------------------------------------
#ifdef __HIPCC__
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Gate non-linearities of the conv epilogues on the hardware transcendental units (v_exp_f32 / v_rcp_f32,
// <= 2 ulp each; absolute error ~2e-7, far inside the 1e-3 px flow tolerance).  The libm forms (expf, a
// correctly rounded divide, OCML tanhf) cost 40-60 VALU instructions per element and showed up as a
// 25 % epilogue tax on the GRU convolutions.
#ifdef OFX_EXACT_GATES   // diagnostic build (tools/epe_curve.py): libm gates, to separate their error from everything else's
__device__ __forceinline__ float ofx_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float ofx_tanh(float x) { return tanhf(x); }
#else
__device__ __forceinline__ float ofx_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float ofx_tanh(float x) {
    const float t = __expf(2.0f * fminf(fmaxf(x, -15.0f), 15.0f));
    return (t - 1.0f) * __builtin_amdgcn_rcpf(t + 1.0f);
}
#endif

// Pillow's DIV255 (Paste.c): a / 255 rounded, exact for a <= 255 * 255
__device__ __forceinline__ unsigned ofx_div255(unsigned a) {
    const unsigned tmp = a + 128u;
    return ((tmp >> 8) + tmp) >> 8;
}

// out[b][x][y] = in[b][y][x] for pixels of type T, a 32 x 32 tile per workgroup of 256 threads; grid (cdiv(W,32), cdiv(H,32), B):
// the step between the horizontal and the vertical passes of the Pillow blurs (handoff.hip: 1-byte pixels, fill.hip: 4-byte)
template <typename T>
__global__ __launch_bounds__(256) void ofx_transpose_tile_kernel(const T* __restrict__ in, T* __restrict__ out, int H, int W) {
    __shared__ T tile[32][33];
    const long b = blockIdx.z;
    const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int j = ty; j < 32; j += 8) {
        const int y = y0 + j, x = x0 + tx;
        if (y < H && x < W) tile[j][tx] = in[(b * H + y) * (long)W + x];
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int x = x0 + j, y = y0 + tx;
        if (y < H && x < W) out[(b * W + x) * (long)H + y] = tile[tx][j];
    }
}

// Keys cubic weights, A = -0.75 (same polynomial form as OpenCV's interpolateCubic)
__device__ __forceinline__ void ofx_cubic_coeffs(float t, float w[4]) {
    const float A = -0.75f;
    float t1 = t + 1.0f;
    w[0] = __fsub_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fsub_rn(__fmul_rn(A, t1), 5.0f * A), t1), 8.0f * A), t1), 4.0f * A);
    w[1] = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(A + 2.0f, t), A + 3.0f), t), t), 1.0f);
    float u = __fsub_rn(1.0f, t);
    w[2] = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(A + 2.0f, u), A + 3.0f), u), u), 1.0f);
    w[3] = __fsub_rn(__fsub_rn(__fsub_rn(1.0f, w[0]), w[1]), w[2]);
}
#endif
