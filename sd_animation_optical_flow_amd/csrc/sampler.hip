// The elementwise chain of one guided DDIM step, one launch:
//
//   ofx_ddim_step   GuidedDDIMSample.p_sample_ddim + the q_sample / mask blend that opens the next iteration of
//                   GuidedDDIMSample.decode (guided_ldm_inpainting.py:28-137), the latent guidance of guided_ldm.py:82-89,123, and
//                   the final blend of img2img_inpaint (guided_ldm_inpainting.py:337-338)
//
// The reference runs torch.cat x2, chunk, the classifier-free-guidance combination, pred_x0, dir_xt, x_prev, then q_sample and the
// mask blend, torch.cat with c_concat and torch.cat x2 again: about two dozen launches and as many temporaries around every UNet
// call.  Here a thread owns one float4 of one pixel row, reads each operand once, and writes the next latent into both
// classifier-free-guidance halves of the UNet's own padded NHWC input (out0, out1: channel slices of that buffer), so a step is
// "UNet, one kernel".  Memory bound and tiny (a 64x96 latent is 96 KiB per operand): one float4 per thread and tensor, a
// grid-stride loop, no LDS.
//
// The arithmetic is the reference's, operation by operation (the header gives the formula); the compiler may fuse a product into the
// sum that follows it, which only removes roundings.  Division is the correctly rounded one.
#include "ofx_internal.h"

#include <algorithm>

namespace {

struct DdimArgs {
    const float *x, *eps_c, *eps_u, *guidance, *gmap, *step_noise, *init, *nmask, *blend_noise;
    float *out0, *out1, *pred_out;
    int ldx, lde, ldg, ldsn, ldi, ldm, ldbn, ldo0, ldo1, ldp;
    ofx_ddim_coef k;
    int blend_only, C;
    long rows;
};

// one float4 of a row as four floats, so the chain below is written once, as a loop over j
__device__ inline void ld4(const float* p, float (&v)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ inline void st4(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }

__global__ __launch_bounds__(256) void ddim_step_kernel(const DdimArgs a) {
    const int cg = a.C / 4;
    const long total = a.rows * cg;
    const ofx_ddim_coef k = a.k;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / cg;
        const int c = (int)(i - row * cg) * 4;
        // every operand of this float4 is read before anything is written: out0 / out1 may be x itself
        float x[4], xp[4], pred[4] = {0.f, 0.f, 0.f, 0.f};
        ld4(a.x + row * a.ldx + c, x);
#pragma unroll
        for (int j = 0; j < 4; ++j) xp[j] = x[j];
        if (!a.blend_only) {
            float e[4];
            ld4(a.eps_c + row * a.lde + c, e);
            if (a.eps_u) {                                             // model_uncond + scale * (model_t - model_uncond)
                float u[4];
                ld4(a.eps_u + row * a.lde + c, u);
#pragma unroll
                for (int j = 0; j < 4; ++j) e[j] = u[j] + k.cfg * (e[j] - u[j]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) pred[j] = (x[j] - k.sqrt_1m_at * e[j]) / k.sqrt_at;
            // guided_ldm.py:82-89, :123.  The reference recomputes eps in every step; without guidance that only rounds eps again,
            // so here it runs with guidance alone
            if (a.guidance) {
                const float g = a.gmap ? a.gmap[row] : k.g;
                float gd[4];
                ld4(a.guidance + row * a.ldg + c, gd);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    pred[j] = pred[j] * (1.0f - g) + gd[j] * g;
                    e[j] = (x[j] - k.sqrt_at * pred[j]) / k.sqrt_1m_at;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) xp[j] = k.sqrt_aprev * pred[j] + k.dir_coef * e[j];
            if (a.step_noise) {
                float n[4];
                ld4(a.step_noise + row * a.ldsn + c, n);
#pragma unroll
                for (int j = 0; j < 4; ++j) xp[j] = xp[j] + k.sigma_t * n[j];
            }
        }
        if (a.nmask) {                                                 // (1 - nmask) * q_sample(init) + nmask * x_dec
            float m[4], q[4];
            ld4(a.nmask + row * a.ldm + c, m);
            ld4(a.init + row * a.ldi + c, q);
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j] = k.sa * q[j];
            if (a.blend_noise) {
                float n[4];
                ld4(a.blend_noise + row * a.ldbn + c, n);
#pragma unroll
                for (int j = 0; j < 4; ++j) q[j] = q[j] + k.s1 * n[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) xp[j] = (1.0f - m[j]) * q[j] + m[j] * xp[j];
        }
        st4(a.out0 + row * a.ldo0 + c, xp);
        if (a.out1) st4(a.out1 + row * a.ldo1 + c, xp);
        if (a.pred_out) st4(a.pred_out + row * a.ldp + c, pred);
    }
}

struct Span {
    const float* p;
    size_t n;     // floats from p to one past the last element touched
};

static inline Span span_of(const float* p, int ld, long rows, int C) { return Span{p, p ? (size_t)(rows - 1) * (size_t)ld + (size_t)C : 0}; }
static inline bool overlaps(Span a, Span b) { return a.p && b.p && a.p < b.p + b.n && b.p < a.p + a.n; }

}  // namespace

extern "C" int ofx_ddim_step(const float* x, int ldx, const float* eps_c, const float* eps_u, int lde, const float* guidance, int ldg,
                             const float* gmap, const float* step_noise, int ldsn, const float* init, int ldi, const float* nmask, int ldm,
                             const float* blend_noise, int ldbn, float* out0, int ldo0, float* out1, int ldo1, float* pred_out, int ldp,
                             const ofx_ddim_coef* coef, int mode, long rows, int C, void* stream) {
    OFX_REQUIRE(x && out0 && coef && rows > 0 && C > 0 && (mode == OFX_DDIM_STEP || mode == OFX_DDIM_BLEND_ONLY), OFX_EINVAL);
    OFX_REQUIRE(rows < (1L << 40) && C < (1 << 24), OFX_EINVAL);
    const bool step = mode == OFX_DDIM_STEP;
    if (step) {
        OFX_REQUIRE(eps_c != nullptr, OFX_EINVAL);
        OFX_REQUIRE(!gmap || guidance, OFX_EINVAL);
    } else {
        // the DDIM part is off: its operands must be absent, and there must be a blend to do
        OFX_REQUIRE(!eps_c && !eps_u && !guidance && !gmap && !step_noise && !pred_out && nmask, OFX_EINVAL);
    }
    OFX_REQUIRE((nmask != nullptr) == (init != nullptr), OFX_EINVAL);
    OFX_REQUIRE(!blend_noise || nmask, OFX_EINVAL);
    OFX_REQUIRE(!nmask || blend_noise || coef->s1 == 0.0f, OFX_EINVAL);
    OFX_REQUIRE(C % 4 == 0, OFX_EALIGN);
    struct Op {
        const float* p;
        int ld;
    };
    const Op ins[] = {{x, ldx}, {eps_c, lde}, {eps_u, lde}, {guidance, ldg}, {step_noise, ldsn}, {init, ldi}, {nmask, ldm}, {blend_noise, ldbn}};
    const Op outs[] = {{out0, ldo0}, {out1, ldo1}, {pred_out, ldp}};
    for (const Op& o : ins) {
        if (!o.p) continue;
        OFX_REQUIRE(o.ld >= C, OFX_EINVAL);
        OFX_REQUIRE(o.ld % 4 == 0 && ofx_aligned16(o.p), OFX_EALIGN);
    }
    for (const Op& o : outs) {
        if (!o.p) continue;
        OFX_REQUIRE(o.ld >= C, OFX_EINVAL);
        OFX_REQUIRE(o.ld % 4 == 0 && ofx_aligned16(o.p), OFX_EALIGN);
    }
    OFX_REQUIRE(!gmap || (((uintptr_t)gmap) & 3u) == 0, OFX_EALIGN);
    // an output may be exactly x (a thread reads its float4 before it writes it); every other overlap is refused
    for (int oi = 0; oi < 3; ++oi) {
        const Op& o = outs[oi];
        if (!o.p) continue;
        const Span so = span_of(o.p, o.ld, rows, C);
        for (const Op& in : ins) {
            const bool in_place = oi < 2 && in.p == x && in.ld == ldx && o.p == x && o.ld == ldx;
            OFX_REQUIRE(in_place || !overlaps(so, span_of(in.p, in.ld, rows, C)), OFX_EINVAL);
        }
        OFX_REQUIRE(!overlaps(so, Span{gmap, gmap ? (size_t)rows : 0}), OFX_EINVAL);
        for (int oj = oi + 1; oj < 3; ++oj) OFX_REQUIRE(!overlaps(so, span_of(outs[oj].p, outs[oj].ld, rows, C)), OFX_EINVAL);
    }
    DdimArgs a;
    a.x = x; a.eps_c = eps_c; a.eps_u = eps_u; a.guidance = guidance; a.gmap = gmap; a.step_noise = step_noise;
    a.init = init; a.nmask = nmask; a.blend_noise = blend_noise;
    a.out0 = out0; a.out1 = out1; a.pred_out = pred_out;
    a.ldx = ldx; a.lde = lde; a.ldg = ldg; a.ldsn = ldsn; a.ldi = ldi; a.ldm = ldm; a.ldbn = ldbn; a.ldo0 = ldo0; a.ldo1 = ldo1; a.ldp = ldp;
    a.k = *coef;
    a.blend_only = step ? 0 : 1;
    a.C = C;
    a.rows = rows;
    hipStream_t s = (hipStream_t)stream;
    const long total = rows * (C / 4);
    OfxProfScope prof("ddim_step", s);
    hipLaunchKernelGGL(ddim_step_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 2048)), dim3(256), 0, s, a);
    return ofx_launch_status();
}
