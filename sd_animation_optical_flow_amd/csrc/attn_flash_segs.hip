// Segmented-K/V instantiations of the fused attention kernels (attn_flash_kernels.h; attn_flash.hip describes the kernels):
// ofx_attention_bnhd_segs reads K and V of every image through a per-image segment table, float32 or float16, in place.
#include "attn_flash_kernels.h"

static_assert(kSegMax == OFX_KV_MAX_SEGMENTS && kSegEntries == OFX_KV_MAX_ENTRIES, "the limits of include/ofx.h");
static_assert(sizeof(FlashSegArgs) <= 4096, "the kernel arguments");

template <bool F16, int SEG>
static int flash_launch_segs_d(const FlashSegArgs& a, int D, hipStream_t s) {
    switch (D) {
#define X(d, bk)                                                              \
    case d:                                                                   \
        if constexpr (F16) return launch_flash_f16<d, bk, true, SEG>(a, s);   \
        else return launch_flash<d, bk, true, SEG>(a, s);
        OFX_FLASH_SIZES(X)
#undef X
    }
    return OFX_EINVAL;
}

// ofx_attention_bnhd_segs after its checks (transformer.hip): image b owns the next counts[b] entries of `segs`, every image sums to Nk
int ofx_attention_flash_segs_launch(const float* q, int ldq, const ofx_kv_segment* segs, const int* counts, int kv_type, const float* bias,
                                    long bias_bstride, float* out, int ldo, int B, int H, int Nq, int Nk, int D, float scale, int precision,
                                    hipStream_t s) {
    FlashSegArgs a{};
    a.q = q; a.bias = bias; a.out = out;
    a.bias_bs = bias_bstride;
    a.BH = B * H; a.Nq = Nq; a.Nk = Nk;
    a.H = H; a.ldq = ldq; a.ldo = ldo;
    if (B > kSegEntries) return OFX_EINVAL;
    int at = 0;
    for (int b = 0; b < B; ++b) {
        if (counts[b] < 1 || counts[b] > kSegMax || at + counts[b] > kSegEntries) return OFX_EINVAL;
        a.first[b] = (unsigned char)at;
        a.cnt[b] = (unsigned char)counts[b];
        int start = 0;
        for (int i = 0; i < counts[b]; ++i, ++at) {
            a.e[at].k = static_cast<const char*>(segs[at].k);
            a.e[at].v = static_cast<const char*>(segs[at].v);
            a.e[at].start = start;
            a.e[at].n = segs[at].n;
            a.e[at].ldk = segs[at].ldk;
            a.e[at].ldv = segs[at].ldv;
            start += segs[at].n;
        }
        if (start != Nk) return OFX_EINVAL;
    }
    if (const int rc = flash_derive(a, scale, precision)) return rc;
    const bool half = kv_type == OFX_KV_F16;
    if (precision == OFX_PREC_F16) {
        OfxProfScope prof(half ? "attn_flash_segs_f16_kv16" : "attn_flash_segs_f16", s);
        prof.flops(4.0 * a.BH * (double)a.Nq * a.Nk * D);
        return half ? flash_launch_segs_d<true, 2>(a, D, s) : flash_launch_segs_d<true, 1>(a, D, s);
    }
    OfxProfScope prof(half ? "attn_flash_segs_kv16" : "attn_flash_segs", s);
    prof.flops(4.0 * a.BH * (double)a.Nq * a.Nk * D);
    return half ? flash_launch_segs_d<false, 2>(a, D, s) : flash_launch_segs_d<false, 1>(a, D, s);
}
