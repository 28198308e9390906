// Native RAFT executor: owns the packed weights on the device and sequences the HIP kernels of one
// `RAFT.forward(test_mode=True)` (RAFT/core/raft.py:86-144) for a batch of frame pairs.
//
// The reference drives ~60 PyTorch ops per refinement iteration from Python; here the whole forward is
// one C call that enqueues ~15 launches per iteration on the caller's stream, with every activation in
// a caller-provided HBM workspace (NHWC fp32):
//
//   encoders   preprocess -> 7x7/s2 conv -> 3 stages x 2 residual blocks -> 1x1 conv
//              fnet: instance-norm statistics kernels + norm/ReLU fused into the next conv's A-load
//              cnet: BatchNorm folded into the conv epilogue (scale/shift), residual add in the epilogue
//   volume     batched fp32-MFMA GEMM + one pooling kernel (4-level pyramid stays resident in HBM)
//   iteration  lookup -> convc1 -> convc2 -> convf1 -> convf2 -> conv -> [zr, q] x2 -> flow head (x2)
//              cat([h, x]) / cat([r*h, x]) / cat([cor, flo]) are channel slices of shared buffers;
//              GRU gates, h update and coords1 += delta live in conv epilogues
//   tail       mask head only on the last iteration (the reference evaluates it on every iteration and
//              discards 19 of 20 results, raft.py:128-139) -> convex upsample -> flow f32[B,H,W,2]
//
// Frame<->keyframe batches share one image (OFX_RAFT_SHARED_IMG2): its feature map is computed once
// and broadcast through a zero batch stride of the correlation GEMM.
#include "ofx_internal.h"

#include <cstdlib>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace {

struct ConvW {
    float* w = nullptr;       // [Cout][Kpad]
    float* wsplit = nullptr;  // the same matrix pre-split into bf16 (hi, lo) quads for the bf16x3 mode
    float* wsplit3 = nullptr; // ... and into (hi, mid | lo) for the bf16x6 mode (ofx_split_conv_weight3: 1.5 x the floats)
    float* scale = nullptr;   // [Cout] or null
    float* shift = nullptr;   // [Cout] or null
    float* wino = nullptr;    // stride-1 3x3 layers (update block, mask.0, the encoders' residual stages): the Winograd F(2x2,3x3)
                              // operand (ofx_wino_conv_weight); the GRU's
                              // per-iteration 1x5 / 5x1 layers: the F(4,5) operand (ofx_wino15_conv_weight); or null
    float* wino4 = nullptr;   // the update block's 3x3 layers, mask.0 and the encoders' stride-1 3x3 layers: the Winograd F(4x4,3x3) operand (ofx_wino44_conv_weight), or null
    int cout = 0, cin = 0, cin_pad = 0, kh = 0, kw = 0;
    long kpad = 0;
    std::string name;         // layer label for the per-layer profile (ofx_prof_enable(2))
};

struct HostTensor {
    const float* data;
    int ndim;
    long shape[4];
    long numel() const {
        long n = 1;
        for (int i = 0; i < ndim; ++i) n *= shape[i];
        return n;
    }
};

constexpr int HD = 128;      // hidden dim (raft.py:38)
constexpr int CD = 128;      // context dim (raft.py:39)
constexpr int FD = 256;      // feature dim (raft.py:54)
constexpr int LEVELS = 4, RADIUS = 4, CORR_CH = LEVELS * (2 * RADIUS + 1) * (2 * RADIUS + 1);   // 324
// row of the lookup's output = convc1's operand: 324 correlation features + 12 zeros.  336 = 21 whole 16-wide K chunks, so every
// chunk of the 1x1 convolution lies inside the row (the scalar-coordinate schedule of conv.hip applies: 116 against 111 TF at the
// same 21 chunks, tools/experiments/README.md) and rows start on 64-byte boundaries; the lookup writes the zeros itself
constexpr int CORR_LD = 336;
// hx row = [h(128) | motion(126) flow(2) | inp(128)] = 384 floats.  The recurrent part (h, motion) is
// contiguous so the per-iteration GRU convolutions read 256 channels; `inp` (the context features) is
// loop-invariant: its contribution to the six GRU convolutions (+ their biases) is computed ONCE per
// forward into `gadd` and enters the per-iteration convolutions as an epilogue addend -- one third of
// the GRU FLOPs leaves the 20-iteration loop.
constexpr int HX_LD = HD + 128 + CD;
constexpr int MOT_OFF = HD;
constexpr int FLOW_OFF = MOT_OFF + 126;
constexpr int INP_OFF = HD + 128;
constexpr int GADD_LD = 2 * (2 * HD + HD);   // [zr1(256) | q1(128) | zr2(256) | q2(128)]
constexpr int FROW = 16;         // floats per flow row: 7 row neighbours x (fx, fy) + 2 zeros -- convf1's operand (flow_head.hip)
constexpr int ENC_CHUNK = 64;          // images per encoder pass (bounds the activation workspace)
// ... fewer for large frames: the widest encoder activation (64 channels at half resolution) must stay
// below the 2 GiB reach of the convolution kernel's 32-bit byte offsets
static inline int enc_chunk(int H, int W) {
    const long per_image = (long)(H / 2) * (W / 2) * 64 * 4;
    const long fit = ((1L << 31) - 4096) / per_image;
    return (int)std::max<long>(1, std::min<long>(ENC_CHUNK, fit));
}

// A single pair at 512x768 gives the convolution kernels 100-400 workgroups per launch on a 256-CU part: the
// machine is under-filled and each launch is latency-bound.  Below this many 1/8-resolution pixels the
// executor therefore runs the independent chains of a forward side by side on separate HIP streams (the
// three encoders; the flow branch of the motion encoder next to the correlation branch).  Large batches fill
// the machine with every launch and stay on one stream.
static inline bool overlap_pays(long M) {
    // (round 6 sweep at 512x768, M = 6144 per frame: four frames 23.9 ms with the side streams / 24.4 without, five 30.9 / 30.3, six
    // 38.0 / 37.7; OFX_OVERLAP_MAX_M overrides)
    static const char* e = getenv("OFX_OVERLAP_MAX_M");
    static const long lim = e ? atol(e) : 28672;
    return M <= lim;
}

struct Carver {
    char* base;
    size_t off = 0, cap;
    Carver(void* b, size_t c) : base((char*)b), cap(c) {}
    float* take(size_t nfloats) {
        size_t bytes = ((nfloats * sizeof(float) + 255) / 256) * 256;
        char* p = base ? base + off : nullptr;
        off += bytes;
        return (float*)p;
    }
};

}  // namespace

struct ofx_raft {
    int variant = 0;   // 0 = basic (raft-things.pth), 1 = small (raft-small.pth): picked from the checkpoint's key set
    std::map<std::string, ConvW> convs;
    // gamma / beta of the context encoder's BatchNorm layers for the batch-statistics mode (OFX_RAFT_BN_BATCH), by norm name
    std::map<std::string, std::pair<float*, float*>> affine;
    std::vector<void*> allocs;
    std::map<std::string, std::pair<void*, size_t>> bufs;
    // side streams for the small-batch schedule (see overlap_pays): independent chains of a forward run
    // concurrently and are joined back into the caller's stream with events
    hipStream_t aux[2] = {nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
};

namespace {

int upload(ofx_raft* r, const std::vector<float>& h, float** d) {
    OFX_HIP_CHECK(hipMalloc((void**)d, h.size() * sizeof(float)));
    r->allocs.push_back(*d);
    OFX_HIP_CHECK(hipMemcpy(*d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// both operand formats of a packed weight matrix: fp32, and the bf16x3 pre-split copy
int upload_weight(ofx_raft* r, const std::vector<float>& packed, ConvW* c) {
    int st = upload(r, packed, &c->w);
    if (st) return st;
    std::vector<float> sp(packed.size());
    st = ofx_split_conv_weight(packed.data(), (long)packed.size(), sp.data());
    if (st) return st;
    st = upload(r, sp, &c->wsplit);
    if (st) return st;
    std::vector<float> sp3(packed.size() * 3 / 2);
    st = ofx_split_conv_weight3(packed.data(), (long)packed.size(), sp3.data());
    if (st) return st;
    return upload(r, sp3, &c->wsplit3);
}

const HostTensor* find(const std::map<std::string, HostTensor>& sd, const std::string& k) {
    auto it = sd.find(k);
    return it == sd.end() ? nullptr : &it->second;
}

// pack one conv (optionally with an eval-mode BatchNorm folded into scale/shift, optionally an
// extra output scale as in `.25 * self.mask(net)`, update.py:135)
int add_conv(ofx_raft* r, const std::map<std::string, HostTensor>& sd, const std::string& name,
             const std::string& store_as, int cin_pad, const std::string& bn, float out_scale,
             std::vector<float>* append_w = nullptr, std::vector<float>* append_shift = nullptr,
             const std::vector<int>* chan_sel = nullptr, bool with_bias = true) {
    const HostTensor* w = find(sd, name + ".weight");
    const HostTensor* b = find(sd, name + ".bias");
    if (!w || !b || w->ndim != 4 || b->ndim != 1 || b->shape[0] != w->shape[0]) return OFX_EKEY;
    ConvW c;
    c.cout = (int)w->shape[0];
    c.cin = (int)w->shape[1];
    c.kh = (int)w->shape[2];
    c.kw = (int)w->shape[3];
    const float* wdata = w->data;
    std::vector<float> wsel;
    if (chan_sel) {   // keep a subset of the input channels, in the given order
        const int full = c.cin, taps = c.kh * c.kw;
        c.cin = (int)chan_sel->size();
        wsel.resize((size_t)c.cout * c.cin * taps);
        for (int o = 0; o < c.cout; ++o)
            for (int ci = 0; ci < c.cin; ++ci) {
                const int src = (*chan_sel)[ci];
                if (src < 0 || src >= full) return OFX_EKEY;
                for (int t = 0; t < taps; ++t)
                    wsel[((size_t)o * c.cin + ci) * taps + t] = w->data[((size_t)o * full + src) * taps + t];
            }
        wdata = wsel.data();
    }
    c.cin_pad = cin_pad > 0 ? cin_pad : ((c.cin + 3) / 4) * 4;
    if (c.cin_pad < c.cin) return OFX_EKEY;
    c.kpad = ofx_pack_conv_weight(nullptr, c.cout, c.cin, c.kh, c.kw, c.cin_pad, nullptr);
    if (c.kpad < 0) return (int)c.kpad;
    std::vector<float> pw((size_t)c.cout * c.kpad);
    ofx_pack_conv_weight(wdata, c.cout, c.cin, c.kh, c.kw, c.cin_pad, pw.data());
    std::vector<float> zero_bias;
    if (!with_bias) zero_bias.assign(c.cout, 0.f);
    HostTensor bz;
    if (!with_bias) {
        bz.data = zero_bias.data();
        bz.ndim = 1;
        bz.shape[0] = c.cout;
        b = &bz;
    }
    std::vector<float> scale, shift(c.cout);
    if (!bn.empty()) {
        const HostTensor* g = find(sd, bn + ".weight");
        const HostTensor* be = find(sd, bn + ".bias");
        const HostTensor* rm = find(sd, bn + ".running_mean");
        const HostTensor* rv = find(sd, bn + ".running_var");
        if (!g || !be || !rm || !rv) return OFX_EKEY;
        if (g->numel() != c.cout || be->numel() != c.cout || rm->numel() != c.cout || rv->numel() != c.cout) return OFX_EKEY;
        scale.resize(c.cout);
        for (int i = 0; i < c.cout; ++i) {
            // F.batch_norm(eval): (x - mean) / sqrt(var + eps) * gamma + beta with x = conv + bias
            const double sc = (double)g->data[i] / std::sqrt((double)rv->data[i] + 1e-5);
            scale[i] = (float)sc;
            shift[i] = (float)(((double)b->data[i] - (double)rm->data[i]) * sc + (double)be->data[i]);
        }
    } else if (out_scale != 1.0f) {
        scale.assign(c.cout, out_scale);
        for (int i = 0; i < c.cout; ++i) shift[i] = b->data[i] * out_scale;
    } else {
        for (int i = 0; i < c.cout; ++i) shift[i] = b->data[i];
    }
    if (append_w) {   // caller concatenates several convs along Cout (GRU z|r)
        append_w->insert(append_w->end(), pw.begin(), pw.end());
        append_shift->insert(append_shift->end(), shift.begin(), shift.end());
        c.w = nullptr;
        c.name = store_as;
        r->convs[store_as] = c;
        return 0;
    }
    int st = upload_weight(r, pw, &c);
    if (st) return st;
    st = upload(r, shift, &c.shift);
    if (st) return st;
    if (!scale.empty()) {
        st = upload(r, scale, &c.scale);
        if (st) return st;
    }
    c.name = store_as;
    r->convs[store_as] = c;
    return 0;
}

// the Winograd operand of an already added 3x3 (F(2x2,3x3), U = G g G^T) or 1x5 / 5x1 (F(4,5), U = G g) layer, made of the input
// channels `sel` (empty: all) of one or more checkpoint convolutions stacked along Cout in the given order (the GRU's z | r): the
// same rows and channels as its direct packing.  conv.hip takes the fused Winograd kernel with it when the grid fills the chip; the
// direct packing stays for every other launch.  wino4: a 3x3 layer gets the F(4x4,3x3) operand as well.
int add_wino(ofx_raft* r, const std::map<std::string, HostTensor>& sd, const std::vector<std::string>& names, const std::vector<int>& sel,
             const std::string& store_as, bool wino4 = false) {
    ConvW& c = r->convs[store_as];
    const int ci = c.cin, taps = c.kh * c.kw;
    const bool k3x3 = c.kh == 3 && c.kw == 3, k1d = (c.kh == 1 && c.kw == 5) || (c.kh == 5 && c.kw == 1);
    if ((!k3x3 && !k1d) || c.cin_pad != ci || (!sel.empty() && (int)sel.size() != ci)) return OFX_EKEY;
    std::vector<float> g;   // [Cout][ci][taps]
    for (const std::string& name : names) {
        const HostTensor* w = find(sd, name + ".weight");
        if (!w || w->ndim != 4 || w->shape[2] != c.kh || w->shape[3] != c.kw) return OFX_EKEY;
        const int co = (int)w->shape[0], full = (int)w->shape[1];
        if (sel.empty() && full != ci) return OFX_EKEY;
        for (int o = 0; o < co; ++o)
            for (int k = 0; k < ci; ++k) {
                const int ch = sel.empty() ? k : sel[k];
                if (ch < 0 || ch >= full) return OFX_EKEY;
                const float* src = w->data + ((size_t)o * full + ch) * taps;
                g.insert(g.end(), src, src + taps);
            }
    }
    if ((long)g.size() != (long)c.cout * ci * taps) return OFX_EKEY;
    auto xf = [&](const float* w, float* out) {
        return k3x3 ? ofx_wino_conv_weight(w, c.cout, ci, out) : ofx_wino15_conv_weight(w, c.cout, ci, c.kh, c.kw, out);
    };
    const long n = xf(nullptr, nullptr);
    if (n < 0) return (int)n;
    std::vector<float> u((size_t)n);
    const long st = xf(g.data(), u.data());
    if (st < 0) return (int)st;
    int up = upload(r, u, &c.wino);
    if (up || !k3x3 || !wino4) return up;
    // the update block's and the encoders' 3x3 layers: the F(4x4,3x3) operand next to it (conv.hip takes it where its grid pays)
    const long n4 = ofx_wino44_conv_weight(nullptr, c.cout, ci, nullptr);
    if (n4 < 0) return (int)n4;
    std::vector<float> u4((size_t)n4);
    const long st4 = ofx_wino44_conv_weight(g.data(), c.cout, ci, u4.data());
    if (st4 < 0) return (int)st4;
    return upload(r, u4, &c.wino4);
}

// `as`: name the packed layers are stored under.  "cnetb" = the context encoder's convolutions WITHOUT the folded running
// statistics, plus gamma / beta of every BatchNorm: the layers of the batch-statistics mode (see ofx_raft_forward).
int build_encoder(ofx_raft* r, const std::map<std::string, HostTensor>& sd, const std::string& enc, bool bn,
                  const std::string& as_ = std::string()) {
    const std::string as = as_.empty() ? enc : as_;
    const bool affine = !as_.empty();
    auto B = [&](const std::string& n) { return bn && !affine ? enc + "." + n : std::string(); };
    auto A = [&](const std::string& n) -> int {   // upload gamma / beta of norm layer `n`
        if (!affine) return 0;
        const HostTensor* g = find(sd, enc + "." + n + ".weight");
        const HostTensor* be = find(sd, enc + "." + n + ".bias");
        if (!g || !be || g->numel() != be->numel() || g->numel() % 4) return OFX_EKEY;
        std::vector<float> hg(g->data, g->data + g->numel()), hb(be->data, be->data + be->numel());
        float *dg = nullptr, *db = nullptr;
        int st = upload(r, hg, &dg);
        if (!st) st = upload(r, hb, &db);
        r->affine[as + "." + n] = std::make_pair(dg, db);
        return st;
    };
    int st = add_conv(r, sd, enc + ".conv1", as + ".conv1", 4, B("norm1"), 1.f);
    if (!st) st = A("norm1");
    if (st) return st;
    for (int li = 1; li <= 3; ++li) {
        for (int bi = 0; bi < 2; ++bi) {
            const std::string p = enc + ".layer" + std::to_string(li) + "." + std::to_string(bi);
            const std::string pa = as + ".layer" + std::to_string(li) + "." + std::to_string(bi);
            const std::string pb = "layer" + std::to_string(li) + "." + std::to_string(bi);
            st = add_conv(r, sd, p + ".conv1", pa + ".conv1", 0, B(pb + ".norm1"), 1.f);
            if (!st) st = A(pb + ".norm1");
            if (st) return st;
            st = add_conv(r, sd, p + ".conv2", pa + ".conv2", 0, B(pb + ".norm2"), 1.f);
            if (!st) st = A(pb + ".norm2");
            if (st) return st;
            // the stride-1 3x3 layers also get the Winograd F(2x2,3x3) and F(4x4,3x3) operands: every conv2, and conv1 but for the
            // first block of a strided stage (conv.hip takes a fused kernel when the grid fills the chip: F(4x4) from 768 workgroups
            // of a 16x32 patch on, with the fused norm, residual merge and statistics of the F(2x2) kernel).
            // OFX_CONV_NO_WINOGRAD_ENC, read once per process at the first engine build: never here
            static const bool no_wino_enc = getenv("OFX_CONV_NO_WINOGRAD_ENC") != nullptr;
            if (!no_wino_enc) {
                if (li == 1 || bi == 1) st = add_wino(r, sd, {p + ".conv1"}, {}, pa + ".conv1", true);
                if (!st) st = add_wino(r, sd, {p + ".conv2"}, {}, pa + ".conv2", true);
                if (st) return st;
            }
            if (li > 1 && bi == 0) {
                st = add_conv(r, sd, p + ".downsample.0", pa + ".down", 0, B(pb + ".norm3"), 1.f);
                if (!st) st = A(pb + ".norm3");
                if (st) return st;
            }
        }
    }
    return add_conv(r, sd, enc + ".conv2", as + ".conv2", 0, "", 1.f);
}

int build_gru(ofx_raft* r, const std::map<std::string, HostTensor>& sd, const std::string& tag) {
    // The reference's GRU input is cat([h, x]) with x = cat([inp, motion]) (update.py:131-133): input
    // channels 0..127 = h, 128..255 = inp, 256..383 = motion.  Split every GRU conv into
    //   * a recurrent part over [h | motion] (256 channels, no bias) evaluated every iteration, and
    //   * a loop-invariant part over [inp] (128 channels, with the bias) evaluated once per forward.
    // z and r share their input: one conv with Cout = 256 ([convz ; convr] rows).
    std::vector<int> rec, inv;
    for (int c = 0; c < HD; ++c) rec.push_back(c);
    for (int c = 0; c < 128; ++c) rec.push_back(HD + CD + c);
    for (int c = 0; c < CD; ++c) inv.push_back(HD + c);
    for (int part = 0; part < 2; ++part) {
        const std::vector<int>* sel = part == 0 ? &rec : &inv;
        const bool bias = part == 1;
        const std::string sfx = part == 0 ? "" : ".inp";
        std::vector<float> w, sh;
        int st = add_conv(r, sd, "update_block.gru.convz" + tag, "gru.z" + tag + sfx, 0, "", 1.f, &w, &sh, sel, bias);
        if (st) return st;
        st = add_conv(r, sd, "update_block.gru.convr" + tag, "gru.r" + tag + sfx, 0, "", 1.f, &w, &sh, sel, bias);
        if (st) return st;
        ConvW c = r->convs["gru.z" + tag + sfx];
        c.cout *= 2;
        st = upload_weight(r, w, &c);
        if (st) return st;
        if (bias) {
            st = upload(r, sh, &c.shift);
            if (st) return st;
        }
        c.name = "gru.zr" + tag + sfx;
        r->convs["gru.zr" + tag + sfx] = c;
        st = add_conv(r, sd, "update_block.gru.convq" + tag, "gru.q" + tag + sfx, 0, "", 1.f, nullptr, nullptr, sel, bias);
        if (st) return st;
        if (part == 0) {   // the per-iteration parts also get the 1D Winograd operand (the once-per-forward .inp parts stay direct)
            st = add_wino(r, sd, {"update_block.gru.convz" + tag, "update_block.gru.convr" + tag}, rec, "gru.zr" + tag);
            if (!st) st = add_wino(r, sd, {"update_block.gru.convq" + tag}, rec, "gru.q" + tag);
            if (st) return st;
        }
    }
    return 0;
}

constexpr size_t SK_BYTES = 65536 + (size_t)1024 * 4 * 64 * 64 * sizeof(float);   // counters + 1024 tiles x 4 splits (conv.hip)

// Where a convolution's epilogue leaves instance-norm partial sums (conv.hip); part == nullptr: it produces none
struct StatsOut {
    float* part = nullptr;
    size_t cap = 0;
};

// One convolution of the engine, operand by operand.  A call site names the operands it uses (designated initialisers, in this order)
// and nothing else; like ConvExtra (ofx_internal.h), nothing reaches the launch except through these fields.
struct ConvArgs {
    const float* in0 = nullptr; int ld0 = 0, c0 = 0;   // the K segments: in0 [.., c0] | in1 [.., c1]
    const float* in1 = nullptr; int ld1 = 0, c1 = 0;
    float* out = nullptr; int ldo = 0;
    int B = 0, Hin = 0, Win = 0, stride = 1;
    int act = OFX_ACT_NONE, epi = OFX_EPI_PLAIN;
    const float* res = nullptr; int ldres = 0;
    const float *nmean = nullptr, *nrstd = nullptr;
    const float* addend = nullptr; int ldadd = 0;
    float *aux_z = nullptr, *aux_rh = nullptr, *aux_h = nullptr; int ldh = 0;
    float *aux_coords = nullptr, *aux_flow4 = nullptr;
    int row_off = 0, rows = 0;                          // a slice of the weight's rows (rows == 0: all of them)
    StatsOut stats;
    hipEvent_t stop_event = nullptr;                    // rides on the kernel's dispatch packet (Streams::arm_*)
};

// What that one launch did with the two optional requests
struct ConvDone {
    int stats_rows = 0;        // rows per image in stats.part, 0 = not produced
    bool stop_taken = false;   // the kernel carries stop_event (false: take the plain edge)
};

// What is per stream and per forward, and nothing per call
struct Launcher {
    hipStream_t s;
    int st = 0;              // sticky: the first error; every later call is skipped
    int precision;           // OFX_PREC_BF16X3 / _BF16X6 / _F16 when the forward was asked for a split-bf16 mode / for fp16
    void* sk_ws;             // split-K scratch of the stream this launcher feeds (null: never split)
    size_t sk_bytes;
    // (fp16 has no split-K kernels and rejects a workspace: its launchers get none, and small grids run unsplit)
    explicit Launcher(hipStream_t s, int precision = OFX_PREC_FP32, void* sk_ws_ = nullptr)
        : s(s), precision(precision), sk_ws(precision == OFX_PREC_F16 ? nullptr : sk_ws_), sk_bytes(sk_ws ? SK_BYTES : 0) {}
    // generic conv launch; all pointer plumbing in one place
    ConvDone conv(const ConvW& c, const ConvArgs& a) {
        ConvDone done;
        if (st) return done;
        ofx_conv_desc d{};
        d.in0 = a.in0; d.ld0 = a.ld0; d.c0 = a.c0;
        d.in1 = a.in1; d.ld1 = a.ld1; d.c1 = a.c1;
        const int cout = a.rows ? a.rows : c.cout;
        const bool whole = a.row_off == 0 && a.rows == 0;
        const bool wsplit = precision == OFX_PREC_BF16X3 && c.wsplit != nullptr;
        // (the three-piece format addresses its lo groups from the end of the whole matrix: row slices keep the on-the-fly split)
        const bool wsplit3 = precision == OFX_PREC_BF16X6 && c.wsplit3 != nullptr && whole;
        d.w = wsplit3 ? c.wsplit3 : (wsplit ? c.wsplit : c.w) + (long)a.row_off * c.kpad;
        d.scale = c.scale ? c.scale + a.row_off : nullptr;
        d.shift = c.shift ? c.shift + a.row_off : nullptr;
        d.out = a.out; d.ldo = a.ldo;
        d.res = a.res; d.ldres = a.ldres;
        d.nmean = a.nmean; d.nrstd = a.nrstd;
        d.addend = a.addend; d.ldadd = a.ldadd;
        d.aux_z = a.aux_z; d.aux_rh = a.aux_rh; d.aux_h = a.aux_h; d.ldh = a.ldh;
        d.aux_coords = a.aux_coords; d.aux_flow4 = a.aux_flow4;
        d.B = a.B; d.Hin = a.Hin; d.Win = a.Win;
        const int padH = c.kh / 2, padW = c.kw / 2;
        d.Hout = (a.Hin + 2 * padH - c.kh) / a.stride + 1;
        d.Wout = (a.Win + 2 * padW - c.kw) / a.stride + 1;
        d.Cout = cout; d.KH = c.kh; d.KW = c.kw; d.stride = a.stride; d.padH = padH; d.padW = padW;
        d.act = a.act; d.epi = a.epi;
        // (fp16: the value that lets the gate epilogues, the norm on load and the epilogue statistics through)
        d.precision = wsplit3 ? OFX_PREC_BF16X6_W : wsplit ? OFX_PREC_BF16X3_W : precision == OFX_PREC_F16 ? OFX_PREC_F16_EPI : precision;
        d.splitk_ws = sk_ws; d.splitk_ws_bytes = sk_bytes;
        d.wino_w = whole ? c.wino : nullptr;
        d.wino4_w = whole ? c.wino4 : nullptr;
        if (a.c0 + a.c1 != c.cin_pad) { st = OFX_EKEY; return done; }
        ofx_prof_set_tag(c.name.c_str());
        ConvExtra x;
        x.stats_part = a.stats.part; x.stats_cap = a.stats.cap; x.stats_rows = a.stats.part ? &done.stats_rows : nullptr;
        x.stop_event = a.stop_event; x.stop_taken = &done.stop_taken;
        st = ofx_conv2d_ex(&d, &x, s);
        ofx_prof_set_tag(nullptr);
        return done;
    }
    // net = tanh(cnet[:, :tanh_rows]), inp = relu(cnet[:, tanh_rows:]) (raft.py:111-114): the context encoder's last convolution as
    // two row slices of one weight, the relu rows landing relu_off floats into the output row.  `a`: the operands both slices share
    void conv_tanh_relu(const ConvW& c, ConvArgs a, int tanh_rows, int relu_off) {
        a.act = OFX_ACT_TANH; a.rows = tanh_rows;
        conv(c, a);
        a.out += relu_off; a.act = OFX_ACT_RELU; a.row_off = tanh_rows; a.rows = c.cout - tanh_rows;
        conv(c, a);
    }
};

struct Streams {
    ofx_raft* r;
    hipStream_t main;
    bool on;
    hipStream_t get(int i) const { return on ? r->aux[i] : main; }
    int fork(int i) const {   // side stream i waits for everything enqueued on the caller's stream so far
        if (!on) return 0;
        OFX_HIP_CHECK(hipEventRecord(r->ev_fork, main));
        OFX_HIP_CHECK(hipStreamWaitEvent(r->aux[i], r->ev_fork, 0));
        return 0;
    }
    int join(int i) const {   // the caller's stream waits for side stream i
        if (!on) return 0;
        OFX_HIP_CHECK(hipEventRecord(r->ev_join[i], r->aux[i]));
        OFX_HIP_CHECK(hipStreamWaitEvent(main, r->ev_join[i], 0));
        return 0;
    }
    // The same two edges with the event riding on a kernel's own dispatch packet (OFX_LAUNCH, ofx_internal.h) instead of a marker
    // packet behind it: arm_*() gives the event (or null) for the launch that ends the producing chain, *_armed() stands where
    // fork() / join() would when that launch took it.
    // On a single 512x768 pair the marker of fork() held the caller's stream for ~7 us per iteration (profiles/r05_single_pair_gap_pairs.txt).
    static bool stop_events() { static const bool off = getenv("OFX_NO_STOP_EVENT") != nullptr; return !off; }
    hipEvent_t arm_fork() const { return on && stop_events() ? r->ev_fork : nullptr; }
    hipEvent_t arm_join(int i) const { return on && stop_events() ? r->ev_join[i] : nullptr; }
    int fork_armed(int i) const { OFX_HIP_CHECK(hipStreamWaitEvent(r->aux[i], r->ev_fork, 0)); return 0; }
    int join_armed(int i) const { OFX_HIP_CHECK(hipStreamWaitEvent(main, r->ev_join[i], 0)); return 0; }
};

// --------------------------------------------------------------------------------------------
// What the four forwards (plain and indexed pairs, of either network) share around their encoders and recurrences: the parsed call,
// the correlation section of the workspace, the pair map, the correlation stage, the output tail and the buffer registration.  Every
// piece is parametrised by data (D, counts, pointers, a flag mask), never by which network calls it.

// One call: the arguments as a C entry point received them, then what parse_call derives from them
struct Call {
    const uint8_t* image1 = nullptr;   // u8 [n1][H][W][3]; the indexed-pairs call: all n_images frames
    const uint8_t* image2 = nullptr;   // u8 [n2][H][W][3]; the indexed-pairs call: unused
    int n_images = 0;                  // the indexed-pairs call: pair b = frames (idx1[b], idx2[b])
    const int *idx1 = nullptr, *idx2 = nullptr;
    int B = 0, H = 0, W = 0, iters = 0, flags = 0;
    float *flow_up = nullptr, *flow_low = nullptr;
    // the first n_warp pairs are warped (all B of a plain call; the indexed-pairs call of the forward-backward confidence, whose reverse
    // flows need no warp, fewer), the rest take the plain upsample
    const uint8_t* warp_frame = nullptr;
    float warp_sign = 1.0f;
    int n_warp = 0;
    uint8_t* warped = nullptr;
    void* workspace = nullptr;
    size_t workspace_bytes = 0;
    hipStream_t s = nullptr;

    int h = 0, w = 0;      // the 1/8 grid
    long N = 0, M = 0;     // its pixels: of one pair, of all B
    int n1 = 0, n2 = 0;    // images on either side: B, 1 when shared, all n_images of the indexed-pairs call
    int bgr = 0, prec = OFX_PREC_FP32;
    bool sh1 = false, sh2 = false, alt = false, warm = false, serial = false, sepst = false;
    // Context-encoder BatchNorm.  Default: the running statistics, folded into the convolutions (a model in .eval(), as PDCNet's
    // own code and canonical RAFT inference run it).  OFX_RAFT_BN_BATCH: the statistics of the image itself -- what
    // `RAFT_2` computes AS WRITTEN: the reference never calls .eval() (ofgen_keyframe_inpaint.py:47-60), so its
    // BatchNorm2d layers (RAFT/core/raft.py:55, extractor.py:118-192) normalise with the statistics of the call's batch,
    // and every call is one image.  Each image of a batch is normalised by itself here (= B reference calls).
    bool bnb = false;
};

// Every argument check of the four forwards, then the derived half of *c.  pairs: the indexed-pairs call; unsupported: the flags the
// network does not take.  Of several violations OFX_EINVAL is reported before OFX_EALIGN (and the workspace's OFX_ENOMEM, known
// only after the network's carve, last).
int parse_call(Call* call, bool pairs, int unsupported) {
    Call& c = *call;
    OFX_REQUIRE(c.image1 && c.workspace && (pairs ? c.idx1 && c.idx2 && c.flow_up : c.image2 && (c.flow_up || c.warped)), OFX_EINVAL);
    OFX_REQUIRE(!(c.flags & OFX_RAFT_FLOW_INIT) || c.flow_low, OFX_EINVAL);   // flow_low carries the initial flow in
    if (c.warped || c.warp_frame || c.n_warp) {
        OFX_REQUIRE(c.warp_frame && c.warped && c.n_warp > 0 && c.n_warp <= c.B && (c.warp_sign == 1.0f || c.warp_sign == -1.0f), OFX_EINVAL);
        OFX_REQUIRE(ofx_upsample_warp_ok(c.n_warp, c.H, c.W) && (((uintptr_t)c.warped) & 3u) == 0, OFX_EINVAL);
    }
    OFX_REQUIRE((!pairs || c.n_images > 0) && c.B > 0 && c.H >= 64 && c.W >= 64 && (c.H % 8) == 0 && (c.W % 8) == 0 && c.iters >= 1, OFX_EINVAL);
    OFX_REQUIRE(!(c.flags & (unsupported | (pairs ? OFX_RAFT_SHARED_IMG1 | OFX_RAFT_SHARED_IMG2 : 0))), OFX_EINVAL);
    for (int b = 0; pairs && b < c.B; ++b)
        OFX_REQUIRE(c.idx1[b] >= 0 && c.idx1[b] < c.n_images && c.idx2[b] >= 0 && c.idx2[b] < c.n_images, OFX_EINVAL);
    if (c.flags & OFX_RAFT_FLOW_INIT) OFX_REQUIRE((((uintptr_t)c.flow_low) & 7u) == 0, OFX_EALIGN);
    OFX_REQUIRE((((uintptr_t)c.workspace) & 255u) == 0, OFX_EALIGN);
    c.h = c.H / 8;
    c.w = c.W / 8;
    c.N = (long)c.h * c.w;
    c.M = (long)c.B * c.N;
    c.bgr = (c.flags & OFX_RAFT_BGR) ? 1 : 0;
    OFX_REQUIRE(!(c.flags & OFX_RAFT_F16) || !(c.flags & (OFX_RAFT_BF16X3 | OFX_RAFT_BF16X6)), OFX_EINVAL);   // one arithmetic for the convolutions
    c.prec = (c.flags & OFX_RAFT_F16) ? OFX_PREC_F16 : (c.flags & OFX_RAFT_BF16X6) ? OFX_PREC_BF16X6 : (c.flags & OFX_RAFT_BF16X3) ? OFX_PREC_BF16X3 : OFX_PREC_FP32;
    c.sh1 = c.flags & OFX_RAFT_SHARED_IMG1;
    c.sh2 = c.flags & OFX_RAFT_SHARED_IMG2;
    c.alt = c.flags & OFX_RAFT_ALT_CORR;
    c.warm = c.flags & OFX_RAFT_FLOW_INIT;
    c.serial = c.flags & OFX_RAFT_SERIAL;
    c.sepst = c.flags & OFX_RAFT_SEPARATE_STATS;
    c.bnb = c.flags & OFX_RAFT_BN_BATCH;
    c.n1 = pairs ? c.n_images : c.sh1 ? 1 : c.B;
    c.n2 = pairs ? c.n_images : c.sh2 ? 1 : c.B;
    return 0;
}

// The correlation section of a workspace: what the correlation stage and the lookups of either network read and write
struct CorrWs {
    float *fmap1, *fmap2, *f2l[LEVELS];
    float* fmap2b;    // image-2 feature maps with rows in the blocked order of the volume's columns (corr.hip)
    float* pyr[LEVELS];
    int* idx_dev;     // image indices per pair for the device (image1's, then image2's; zeros for a shared frame), see make_pair_map
    void* warp_pad;   // zero-bordered RGBX copy of the frame the tail warps (ofx_raft_forward_warp)
};

// n1 / n2 feature maps of D channels (n_images > 0, the indexed-pairs layout: n1 = n_images maps serve both sides, n2 = 0), the pooled
// levels of image 2 (alt, the volume-free mode) or its blocked copy and the pyramid of B pairs, then idx_slots ints for the pair map
void carve_corr(CorrWs* w, Carver& c, int D, int B, int H, int W, long n1, long n2, int n_images, bool alt, int idx_slots) {
    const int h = H / 8, wd = W / 8;
    const long N = (long)h * wd;
    const long M = (long)B * N;
    w->fmap1 = c.take((size_t)n1 * N * D);
    w->fmap2 = n2 ? c.take((size_t)n2 * N * D) : w->fmap1;   // directly behind fmap1: fold_key lets the shared key frame's map land there
    if (alt) {
        // volume-free mode: the pooled levels of fmap2, once per unique image, and no pyramid at all
        w->f2l[0] = w->fmap2;
        for (int l = 1; l < LEVELS; ++l) w->f2l[l] = c.take((size_t)(n_images > 0 ? n_images : n2) * (h >> l) * (wd >> l) * D);
    } else {
        w->fmap2b = c.take((size_t)(n_images > 0 ? n_images : n2) * ofx_corr_slice_floats_l(h, wd) * D);
        for (int l = 0; l < LEVELS; ++l) w->pyr[l] = c.take((size_t)M * ofx_corr_slice_floats_l(h >> l, wd >> l));
    }
    w->idx_dev = idx_slots ? (int*)c.take((size_t)idx_slots) : nullptr;
    w->warp_pad = c.take(ofx_warp_pad_bytes(H, W) / sizeof(float) + 4);
}

// Which image of fmap1 / fmap2 each pair reads: device arrays for the tiled lookup and the split-plane volume (null = pair b reads image
// b), and the same on the host (arrays of the indexed-pairs call, or the shared flags) for the per-pixel kernel and the per-pair GEMMs
struct PairMap {
    const int *d1 = nullptr, *d2 = nullptr, *h1 = nullptr, *h2 = nullptr;
    bool sh1 = false, sh2 = false;
    // from one pair's image to the next, given the size of one: nothing where the pairs share the image or find it by index
    long step1(long per_image) const { return sh1 || h1 ? 0 : per_image; }
    long step2(long per_image) const { return sh2 || h2 ? 0 : per_image; }
};

// dev1 / dev2: the device reads that side's indices -- the lists of the indexed-pairs call, copied into idx_dev; zeros for a shared
// frame (the image index of every pair)
int make_pair_map(PairMap* pm, const Call& c, int* idx_dev, bool dev1, bool dev2) {
    pm->h1 = c.idx1; pm->h2 = c.idx2;
    pm->sh1 = c.sh1; pm->sh2 = c.sh2;
    if (c.idx1) {
        if (dev1) OFX_HIP_CHECK(hipMemcpyAsync(idx_dev, c.idx1, sizeof(int) * c.B, hipMemcpyHostToDevice, c.s));
        if (dev2) OFX_HIP_CHECK(hipMemcpyAsync(idx_dev + c.B, c.idx2, sizeof(int) * c.B, hipMemcpyHostToDevice, c.s));
        pm->d1 = dev1 ? idx_dev : nullptr; pm->d2 = dev2 ? idx_dev + c.B : nullptr;
    } else if ((dev1 && c.sh1) || (dev2 && c.sh2)) {
        OFX_HIP_CHECK(hipMemsetAsync(idx_dev, 0, sizeof(int) * c.B, c.s));
        pm->d1 = dev1 && c.sh1 ? idx_dev : nullptr; pm->d2 = dev2 && c.sh2 ? idx_dev : nullptr;
    }
    return 0;
}

// OFX_LOCAL_CORR_NO_TILED=1: every volume-free lookup of the engine on the per-pixel kernel of ofx_local_corr_fwd (diagnostic)
static bool local_corr_tiled() {
    static const bool off = [] { const char* e = getenv("OFX_LOCAL_CORR_NO_TILED"); return e && *e && *e != '0'; }();
    return !off;
}

// correlation features of all LEVELS levels at coords, without a volume, into the lookup rows (ld floats per pixel)
static int alt_lookup(const float* fmap1, float* const* f2l, const PairMap& ix, const float* coords, float* corr, int ld, int B, int h, int w,
                      int D, int radius, hipStream_t s) {
    const float scale = 1.0f / std::sqrt((float)D);
    if (local_corr_tiled()) return ofx_local_corr_tiled_launch(fmap1, f2l, ix.d1, ix.d2, coords, corr, ld, B, h, w, D, radius, LEVELS, scale, s);
    const long N = (long)h * w;
    const int rd2 = (2 * radius + 1) * (2 * radius + 1);
    const bool indexed = ix.h1 || ix.h2 || ix.sh1 || ix.sh2;
    for (int l = 0; l < LEVELS; ++l) {
        const long n2 = (long)(h >> l) * (w >> l) * D;
        for (int b = 0; b < (indexed ? B : 1); ++b) {   // the per-pixel kernel pairs image b with image b: one launch per indexed pair
            const long i1 = ix.h1 ? ix.h1[b] : ix.sh1 ? 0 : b, i2 = ix.h2 ? ix.h2[b] : ix.sh2 ? 0 : b;
            const int st = ofx_local_corr_launch(fmap1 + i1 * N * D, f2l[l] + i2 * n2, coords + (long)b * N * 2, corr + (long)b * N * ld + (long)l * rd2,
                                                 N * ld, 0, 1, ld, indexed ? 1 : B, h, w, h >> l, w >> l, D, 1, radius, scale, 1.0f / (float)(1 << l), s);
            if (st) return st;
        }
    }
    return 0;
}

// The all-pairs volume as a batched 1x1 convolution (conv.hip's generic GEMM), for both networks: level 0 (and level 1 out of the
// accumulators where the shape allows: level 0 is then never read back) of nz pairs.  f1: rows [N][D] at a_zs floats per pair; f2b:
// image 2's rows in the blocked order of the volume's columns [Nb][D] at w_zs per pair -- a zero stride broadcasts a shared feature
// map across the batch.  *fused tells the pooling launch whether level 1 is already there.
// One pair at a time (the indexed-pairs calls) passes nz = 1 and that pair's own pointers: conv.hip reads nz as `nz > 1 ? nz : 1` and
// drops the three batch strides of a single z, and the pool's stride is only ever multiplied by z = 0 -- the launch is the one a
// descriptor without any of them gives.
static int volume_gemm(const float* f1, long a_zs, const float* f2b, long w_zs, float* l0, float* l1, int nz, int h, int w, int D,
                       int precision, bool* fused, hipStream_t s) {
    const long N = (long)h * w, Nb = ofx_corr_slice_floats_l(h, w), slice1 = ofx_corr_slice_floats_l(h >> 1, w >> 1);
    ofx_conv_desc d{};
    d.in0 = f1; d.ld0 = D; d.c0 = D;
    d.w = f2b;
    d.out = l0; d.ldo = (int)Nb;
    d.nz = nz; d.a_zs = a_zs; d.w_zs = w_zs; d.o_zs = N * Nb;
    d.B = 1; d.Hin = h; d.Win = w; d.Hout = h; d.Wout = w; d.Cout = (int)Nb;
    d.KH = 1; d.KW = 1; d.stride = 1;
    d.act = OFX_ACT_NONE; d.epi = OFX_EPI_PLAIN;
    d.precision = precision;
    *fused = ofx_corr_volpool_ok(h, w) && Nb % 128 == 0 && N * slice1 * 4 < (1L << 31) - 64;   // (every arithmetic since round 4)
    ConvExtra x;
    x.alpha = 1.0f / std::sqrt((float)D);
    if (*fused) x.pool = {l1, N * slice1, (w + 7) >> 3, ((w >> 1) + 7) >> 3, (int)slice1};
    return ofx_conv2d_ex(&d, &x, s);
}

// The correlation stage: what the lookups of the recurrence read, from the feature maps of D channels.  Three forms --
//   c.alt        volume-free: the pooled levels of every image-2 map, and no volume
//   planes > 0   the volume on the A-stationary kernel (corr_split.hip): every image split into `planes` bf16 planes (1: exact fp32)
//                once per role -- rows scaled in pixel order, columns in quad order -- in plane_scratch, then ONE launch over all pairs
//   planes == 0  the volume on conv.hip's generic GEMM: the blocked copy of every image-2 map, one batched launch -- or, where the pairs
//                find their images by index, one N x Nb GEMM per pair straight from the shared feature maps
// and, for both volume forms, the pooling launch of the remaining pyramid levels.  The caller decides `planes`.
int correlate(const Call& c, const CorrWs& ws, const PairMap& pm, int D, int prec, int planes, void* plane_scratch) {
    const int B = c.B, h = c.h, w = c.w;
    const long N = c.N;
    hipStream_t s = c.s;
    int st = 0;
    if (c.alt) {
        for (int l = 1; l < LEVELS && !st; ++l) st = ofx_avgpool2_nhwc(ws.f2l[l - 1], ws.f2l[l], c.n2, h >> (l - 1), w >> (l - 1), D, s);
        return st;
    }
    bool fused = false;
    if (prec == OFX_PREC_F16) prec = OFX_PREC_FP32;   // fp16 rounds the convolutions' operands only: the volume stays exact fp32 (raft.py:102-103, .float())
    if (planes) {
        char* pl = (char*)plane_scratch;
        const long ib = (long)ofx_corr_planes_bytes(h, w, planes);
        st = ofx_corr_split_planes(ws.fmap1, pl, c.n1, h, w, planes, 0, 1.0f / std::sqrt((float)D), s);
        if (!st) st = ofx_corr_split_planes(ws.fmap2, pl + ib * c.n1, c.n2, h, w, planes, 1, 1.0f, s);
        if (!st)
            st = ofx_corr_vol_split_launch(pl, pl + ib * c.n1, pm.d1, pm.d2, pm.step1(ib), pm.step2(ib), ws.pyr[0], ws.pyr[1], B, h, w, planes, s);
        fused = true;
    } else {
        // the volume's columns in blocked order: permute the rows of the B operand once (6.3 MB per image)
        const long Nb = ofx_corr_slice_floats_l(h, w), slice1 = ofx_corr_slice_floats_l(h >> 1, w >> 1);
        st = ofx_corr_block_rows(ws.fmap2, ws.fmap2b, c.n2, h, w, D, s);
        if (!st && !pm.h1)
            st = volume_gemm(ws.fmap1, pm.step1(N * D), ws.fmap2b, pm.step2(Nb * D), ws.pyr[0], ws.pyr[1], B, h, w, D, prec, &fused, s);
        for (int b = 0; b < B && !st && pm.h1; ++b)
            st = volume_gemm(ws.fmap1 + (long)pm.h1[b] * N * D, 0, ws.fmap2b + (long)pm.h2[b] * Nb * D, 0, ws.pyr[0] + (long)b * N * Nb,
                             ws.pyr[1] + (long)b * N * slice1, 1, h, w, D, prec, &fused, s);
    }
    if (!st) st = ofx_corr_pool_launch(ws.pyr[0], ws.pyr[1], ws.pyr[2], ws.pyr[3], B, h, w, LEVELS, s, fused);
    return st;
}

// The tail of a forward: the final coords1 upsampled to flow_up -- the convex upsample with the mask head's weights, upflow8
// (utils/utils.py:80-82) with a null mask, as RAFT.forward does when up_mask is None -- with the backward warp of c.warp_frame in the same
// pass for the first c.n_warp pairs (the flow is in registers right there; flow_up is then written only if wanted), and flow_low
int finish_flow(const Call& c, const float* coords1, const float* mask, const void* warp_pad) {
    const int B = c.B, h = c.h, w = c.w, nw = c.n_warp;
    const long N = c.N;
    int st = 0;
    if (nw > 0)
        st = mask ? ofx_upsample_warp_launch(coords1, mask, c.flow_up, warp_pad, c.warped, nw, h, w, c.warp_sign, c.s)
                  : ofx_upflow8_warp_launch(coords1, c.flow_up, warp_pad, c.warped, nw, h, w, c.warp_sign, c.s);
    if (!st && nw < B) {
        if (!c.flow_up) return OFX_EINVAL;
        st = mask ? ofx_upsample_flow(coords1 + (long)nw * N * 2, mask + (long)nw * N * 576, c.flow_up + (long)nw * N * 128, B - nw, h, w, c.s)
                  : ofx_upflow8(coords1 + (long)nw * N * 2, c.flow_up + (long)nw * N * 128, B - nw, h, w, c.s);
    }
    if (st) return st;
    if (c.flow_low) return ofx_coords_to_flow(coords1, c.flow_low, B, h, w, c.s);
    return 0;
}

// The intermediates of a plain forward, by name (ofx_raft_buffer): feature maps of D channels, the recurrence's rows at their widths, the
// pyramid levels in their blocked layout (ofx.h) unless the call was volume-free; mask only where the network has a mask head
void register_buffers(ofx_raft* r, const Call& c, const CorrWs& ws, int D, float* hx, int hx_ld, float* coords1, float* corr, int corr_ld,
                      float* mask) {
    r->bufs.clear();
    auto reg = [&](const char* k, float* p, size_t nf) { r->bufs[k] = std::make_pair((void*)p, nf); };
    reg("fmap1", ws.fmap1, (size_t)c.n1 * c.N * D);
    reg("fmap2", ws.fmap2, (size_t)c.n2 * c.N * D);
    reg("hx", hx, (size_t)c.M * hx_ld);
    reg("coords1", coords1, (size_t)c.M * 2);
    reg("corr", corr, (size_t)c.M * corr_ld);
    if (mask) reg("mask", mask, (size_t)c.M * 576);
    if (!c.alt)
        for (int l = 0; l < LEVELS; ++l) {
            char nm[8];
            snprintf(nm, sizeof nm, "pyr%d", l);
            reg(nm, ws.pyr[l], (size_t)c.M * ofx_corr_slice_floats_l(c.h >> l, c.w >> l));
        }
}

// --------------------------------------------------------------------------------------------
// The basic network (raft-things.pth)

struct EncBufs {
    void* sk = nullptr;      // split-K scratch of the stream this encoder chain runs on
    float *x0, *X, *Y, *R1, *R2, *R3;
    float* stats;     // 6 x [chunk][128] floats (mean/rstd for up to 3 norms)
    float* scratch;   // inorm partial sums
    float* spart;     // instance-norm partial sums written by the convolution epilogues: [chunk][rows][C][2]
    size_t spart_floats;
};

}  // namespace

// --------------------------------------------------------------------------------------------
static int run_encoder(ofx_raft* r, const std::string& enc, bool bn, const uint8_t* imgs, int n, int H, int W,
                       int bgr, const EncBufs& eb, float* out, int out_ld, bool split_tanh_relu, int relu_off, hipStream_t s,
                       int precision = OFX_PREC_FP32, bool separate_stats = false, const uint8_t* extra = nullptr) {
    // `extra`: one more image appended to the chunk (the shared key frame riding with the frames: see basic_forward)
    // `out`: [n*h*w][out_ld]; fnet writes 256 channels; cnet writes tanh(0:128) | relu(128:256)
    Launcher L(s, precision, eb.sk);
    const int H2 = H / 2, W2 = W / 2;
    const int SC = (ENC_CHUNK + 1) * 128;   // floats per stats vector slot
    float* m1 = eb.stats + 0 * SC; float* s1 = eb.stats + 1 * SC;
    float* m2 = eb.stats + 2 * SC; float* s2 = eb.stats + 3 * SC;
    float* m3 = eb.stats + 4 * SC; float* s3 = eb.stats + 5 * SC;
    auto C = [&](const std::string& k) -> const ConvW& { return r->convs[enc + "." + k]; };
    int st = ofx_preprocess_u8(imgs, eb.x0, (long)n * H * W, bgr, s);
    if (st) return st;
    if (extra) {
        st = ofx_preprocess_u8(extra, eb.x0 + (long)n * H * W * 4, (long)H * W, bgr, s);
        if (st) return st;
        ++n;
    }
    // statistics of the tensor x a convolution has just written: from its epilogue's partial sums when it produced them (`rows`: that
    // conv()'s stats_rows), with a pass of their own over x otherwise.
    // `norm`: the layer's name -- for "cnetb" (BatchNorm on per-image statistics) its gamma / beta are folded into (mean, rstd)
    auto stats = [&](int rows, const float* x, long HW, int ch, float* mean, float* rstd, const std::string& norm) {
        if (L.st) return;
        const float *gamma = nullptr, *beta = nullptr;
        auto af = r->affine.find(enc + "." + norm);
        if (af != r->affine.end()) { gamma = af->second.first; beta = af->second.second; }
        if (rows > 0) L.st = ofx_inorm_finalize_part(eb.spart, mean, rstd, n, rows, HW, ch, 1e-5f, s, gamma, beta);
        else L.st = ofx_inorm_stats_affine(x, ch, mean, rstd, eb.scratch, n, HW, ch, 1e-5f, gamma, beta, s);
    };
    static const bool no_epi_stats = getenv("OFX_NO_EPI_STATS") != nullptr;     // diagnostic: always the separate statistics pass
    // the `.stats` of a convolution whose output is normalised next
    const StatsOut epi_stats = no_epi_stats || separate_stats ? StatsOut{} : StatsOut{eb.spart, eb.spart_floats};
    float* X = eb.X;
    float* Y = eb.Y;
    // instance norm: the stem's normalised output is never materialised.  Its raw output stays in X with its statistics in (m3, s3)
    // -- free until the first strided block -- and both of its consumers apply relu(norm(.)) on the fly: layer1.0.conv1 in its
    // operand staging (like every conv2), layer1.0's residual merge inside its inorm_apply (relu bit 1).  One full-resolution
    // read + write pass less per encoder.
    bool stem_raw = false;
    if (!bn) {
        const int rows = L.conv(C("conv1"), {.in0 = eb.x0, .ld0 = 4, .c0 = 4, .out = X, .ldo = 64, .B = n, .Hin = H, .Win = W, .stride = 2,
                                             .stats = epi_stats}).stats_rows;
        stats(rows, X, (long)H2 * W2, 64, m3, s3, "norm1");
        stem_raw = true;
    } else {
        L.conv(C("conv1"), {.in0 = eb.x0, .ld0 = 4, .c0 = 4, .out = X, .ldo = 64, .B = n, .Hin = H, .Win = W, .stride = 2, .act = OFX_ACT_RELU});
    }
    int hin = H2, win = W2, cin = 64;
    const int dims[3] = {64, 96, 128};
    for (int li = 1; li <= 3; ++li) {
        const int dim = dims[li - 1];
        for (int bi = 0; bi < 2; ++bi) {
            const int stride = (li > 1 && bi == 0) ? 2 : 1;
            const int ho = hin / stride, wo = win / stride;
            const std::string p = "layer" + std::to_string(li) + "." + std::to_string(bi);
            if (!bn) {
                int rows = L.conv(C(p + ".conv1"), {.in0 = X, .ld0 = cin, .c0 = cin, .out = eb.R1, .ldo = dim, .B = n, .Hin = hin, .Win = win,
                                                    .stride = stride, .nmean = stem_raw ? m3 : nullptr, .nrstd = stem_raw ? s3 : nullptr,
                                                    .stats = epi_stats}).stats_rows;
                stats(rows, eb.R1, (long)ho * wo, dim, m1, s1, p + ".norm1");
                // norm1 + ReLU fused into conv2's operand load
                rows = L.conv(C(p + ".conv2"), {.in0 = eb.R1, .ld0 = dim, .c0 = dim, .out = eb.R2, .ldo = dim, .B = n, .Hin = ho, .Win = wo,
                                                .nmean = m1, .nrstd = s1, .stats = epi_stats}).stats_rows;
                stats(rows, eb.R2, (long)ho * wo, dim, m2, s2, p + ".norm2");
                if (stride == 2) {
                    rows = L.conv(C(p + ".down"), {.in0 = X, .ld0 = cin, .c0 = cin, .out = eb.R3, .ldo = dim, .B = n, .Hin = hin, .Win = win,
                                                   .stride = 2, .stats = epi_stats}).stats_rows;
                    stats(rows, eb.R3, (long)ho * wo, dim, m3, s3, p + ".norm3");
                    if (!L.st) L.st = ofx_inorm_apply(eb.R2, m2, s2, eb.R3, m3, s3, Y, n, (long)ho * wo, dim, 1, s);
                } else {
                    if (!L.st)
                        L.st = ofx_inorm_apply(eb.R2, m2, s2, X, stem_raw ? m3 : nullptr, stem_raw ? s3 : nullptr, Y, n, (long)ho * wo, dim,
                                               stem_raw ? 3 : 1, s);
                }
                stem_raw = false;
            } else {
                L.conv(C(p + ".conv1"), {.in0 = X, .ld0 = cin, .c0 = cin, .out = eb.R1, .ldo = dim, .B = n, .Hin = hin, .Win = win,
                                         .stride = stride, .act = OFX_ACT_RELU});
                const float* res = X;
                if (stride == 2) {
                    L.conv(C(p + ".down"), {.in0 = X, .ld0 = cin, .c0 = cin, .out = eb.R3, .ldo = dim, .B = n, .Hin = hin, .Win = win, .stride = 2});
                    res = eb.R3;
                }
                L.conv(C(p + ".conv2"), {.in0 = eb.R1, .ld0 = dim, .c0 = dim, .out = Y, .ldo = dim, .B = n, .Hin = ho, .Win = wo,
                                         .act = OFX_ACT_RELU, .res = res, .ldres = dim});
            }
            std::swap(X, Y);
            hin = ho; win = wo; cin = dim;
        }
    }
    const ConvArgs last{.in0 = X, .ld0 = 128, .c0 = 128, .out = out, .ldo = out_ld, .B = n, .Hin = hin, .Win = win};
    if (!split_tanh_relu) L.conv(C("conv2"), last);
    else L.conv_tanh_relu(C("conv2"), last, HD, relu_off);
    return L.st;
}

// workspace layout shared by the size query and the forward
struct RaftWs : CorrWs {
    EncBufs eb[3];    // [1], [2] only exist (else alias [0]) when the encoders may run concurrently
    void* sk[3];      // split-K scratch per stream (small batches only; null otherwise)
    float* ctx;       // indexed-pairs mode: per-image context features [n][N][256] (tanh | relu halves)
    float *hx, *gadd, *coords1, *frows, *corr, *c1, *corflo, *f1, *z, *rh, *mask;
    size_t bytes;
};

// n_images > 0 selects the indexed-pairs layout: one feature map + one context map per unique image
static RaftWs carve(void* base, size_t cap, int B, int H, int W, int flags, int n_images = 0) {
    RaftWs w{};
    Carver c(base, cap);
    const int h = H / 8, wd = W / 8;
    const long N = (long)h * wd;
    const long M = (long)B * N;
    const int most = n_images > 0 ? n_images : 2 * B;
    const int nch = std::min(enc_chunk(H, W) + 1, most);   // + 1: the shared key frame rides in the last chunk of the frames (fold_key)
    const long half = (long)(H / 2) * (W / 2) * 64;
    for (int e = 0; e < 3; ++e) w.sk[e] = overlap_pays(M) ? (void*)c.take(SK_BYTES / sizeof(float)) : nullptr;
    for (int e = 0; e < 3; ++e) {
        if (e > 0 && !overlap_pays(M)) {
            w.eb[e] = w.eb[0];
            continue;
        }
        EncBufs& eb = w.eb[e];
        eb.sk = w.sk[e];
        eb.x0 = c.take((size_t)nch * H * W * 4);
        eb.X = c.take((size_t)nch * half);
        eb.Y = c.take((size_t)nch * half);
        eb.R1 = c.take((size_t)nch * half);
        eb.R2 = c.take((size_t)nch * half);
        eb.R3 = c.take((size_t)nch * (H / 4) * (W / 4) * 96);
        eb.stats = c.take((size_t)6 * (ENC_CHUNK + 1) * 128);
        eb.scratch = c.take((size_t)(ENC_CHUNK + 1) * 64 * 128 * 2 * 2);   // doubles: chunk x slices x C x {sum, sumsq}
        // one (sum, sumsq) pair per channel and 32 tile rows at most: the half-resolution 64-channel stage bounds it
        eb.spart_floats = (size_t)nch * (H / 2) * (W / 2) * 4 + 4096;
        eb.spart = c.take(eb.spart_floats);
    }
    long n1 = (flags & OFX_RAFT_SHARED_IMG1) ? 1 : B, n2 = (flags & OFX_RAFT_SHARED_IMG2) ? 1 : B;
    if (n_images > 0) {
        n1 = n_images;
        n2 = 0;
        w.ctx = c.take((size_t)n_images * N * (HD + CD));
    }
    // index slots: the indexed-pairs call's image1 indices (ofx_ctx_gather reads them in either mode), then its image2 indices; the
    // volume-free plain call's zeros for a shared frame
    const bool alt = flags & OFX_RAFT_ALT_CORR;
    carve_corr(&w, c, FD, B, H, W, n1, n2, n_images, alt, n_images > 0 ? 2 * B : alt ? B : 0);
    w.hx = c.take((size_t)M * HX_LD);
    w.gadd = c.take((size_t)M * GADD_LD);
    w.coords1 = c.take((size_t)M * 2);
    w.frows = c.take((size_t)M * FROW);
    w.corr = c.take((size_t)M * CORR_LD);
    w.c1 = c.take((size_t)M * 256);
    w.corflo = c.take((size_t)M * 256);
    w.f1 = c.take((size_t)M * 128);
    w.z = c.take((size_t)M * HD);
    w.rh = c.take((size_t)M * HD);
    w.mask = c.take((size_t)M * 576);
    w.bytes = c.off;
    return w;
}

// everything after the feature / context encoders and the correlation volume: state init, the loop-invariant
// GRU terms, `iters` refinement iterations, mask head (the convex upsample is finish_flow's)
// c.warm: flow_low holds the initial flow (OFX_RAFT_FLOW_INIT); it is read here and overwritten with the final flow by finish_flow
static int run_recurrence(ofx_raft* r, const RaftWs& ws, const Call& c, const PairMap& aix, bool overlap) {
    const int B = c.B, h = c.h, w = c.w, iters = c.iters, precision = c.prec;
    const bool alt = c.alt, warm = c.warm;
    float* flow_low = c.flow_low;
    hipStream_t s = c.s;
    const long N = c.N;
    int st = 0;
    st = warm ? ofx_init_state_warm(ws.coords1, ws.frows, ws.hx, HX_LD, FLOW_OFF, false, flow_low, B, h, w, s)
              : ofx_init_state(ws.coords1, ws.frows, ws.hx, HX_LD, FLOW_OFF, B, h, w, s);
    if (st) return st;
    {   // loop-invariant GRU terms: conv(W[:, inp], inp) + bias for z|r and q of both passes
        Launcher G(s, precision, ws.sk[0]);
        const char* names[4] = {"gru.zr1.inp", "gru.q1.inp", "gru.zr2.inp", "gru.q2.inp"};
        const int offs[4] = {0, 2 * HD, 3 * HD, 5 * HD};
        for (int i = 0; i < 4; ++i)
            G.conv(r->convs[names[i]], {.in0 = ws.hx + INP_OFF, .ld0 = HX_LD, .c0 = CD, .out = ws.gadd + offs[i], .ldo = GADD_LD, .B = B, .Hin = h, .Win = w});
        if (G.st) return G.st;
    }

    if (alt) OFX_HIP_CHECK(hipMemsetAsync(ws.corr, 0, (size_t)B * N * CORR_LD * sizeof(float), s));   // (the pad columns: the volume-free kernel writes 324 of 336)
    Launcher L(s, precision, ws.sk[0]);
    const Streams S{r, s, overlap};
    // flow branch of the motion encoder: independent of the correlation branch, with its own scratch when it runs concurrently
    Launcher LF(S.get(0), precision, overlap ? ws.sk[1] : ws.sk[0]);
    auto C = [&](const char* k) -> const ConvW& { return r->convs[k]; };
    const float* pyr_c[LEVELS] = {ws.pyr[0], ws.pyr[1], ws.pyr[2], ws.pyr[3]};
    bool fork_on_kernel = false;   // the previous iteration's flow head carries ev_fork
    for (int it = 0; it < iters && !L.st; ++it) {
        // flow features (update.py:93-94) on the side stream, from the flow the previous iteration left
        if ((L.st = fork_on_kernel ? S.fork_armed(0) : S.fork(0))) break;
        LF.conv(C("convf1"), {.in0 = ws.frows, .ld0 = FROW, .c0 = FROW, .out = ws.f1, .ldo = 128, .B = B, .Hin = h, .Win = w,
                              .act = OFX_ACT_RELU});   // 7x1 over the flow rows
        const bool join_on_kernel = LF.conv(C("convf2"), {.in0 = ws.f1, .ld0 = 128, .c0 = 128, .out = ws.corflo + 192, .ldo = 256, .B = B,
                                                          .Hin = h, .Win = w, .act = OFX_ACT_RELU, .stop_event = S.arm_join(0)}).stop_taken;
        if ((L.st = LF.st)) break;
        // correlation features at the current estimate
        if (!alt) {
            L.st = ofx_corr_lookup_pad(pyr_c, ws.coords1, ws.corr, CORR_LD, CORR_LD - CORR_CH, B, h, w, LEVELS, RADIUS, s);
        } else {
            L.st = alt_lookup(ws.fmap1, ws.f2l, aix, ws.coords1, ws.corr, CORR_LD, B, h, w, FD, RADIUS, s);
        }
        // motion encoder (update.py:88-97)
        L.conv(C("convc1"), {.in0 = ws.corr, .ld0 = CORR_LD, .c0 = CORR_LD, .out = ws.c1, .ldo = 256, .B = B, .Hin = h, .Win = w, .act = OFX_ACT_RELU});
        L.conv(C("convc2"), {.in0 = ws.c1, .ld0 = 256, .c0 = 256, .out = ws.corflo, .ldo = 256, .B = B, .Hin = h, .Win = w, .act = OFX_ACT_RELU});
        if (!L.st) L.st = join_on_kernel ? S.join_armed(0) : S.join(0);
        L.conv(C("conv"), {.in0 = ws.corflo, .ld0 = 256, .c0 = 256, .out = ws.hx + MOT_OFF, .ldo = HX_LD, .B = B, .Hin = h, .Win = w,
                           .act = OFX_ACT_RELU});
        // SepConvGRU (update.py:44-60): horizontal then vertical pass
        for (int pass = 1; pass <= 2; ++pass) {
            const char* zr = pass == 1 ? "gru.zr1" : "gru.zr2";
            const char* q = pass == 1 ? "gru.q1" : "gru.q2";
            const float* g = ws.gadd + (pass - 1) * (3 * HD);
            L.conv(C(zr), {.in0 = ws.hx, .ld0 = HX_LD, .c0 = 2 * HD, .B = B, .Hin = h, .Win = w, .epi = OFX_EPI_GRU_ZR, .addend = g,
                           .ldadd = GADD_LD, .aux_z = ws.z, .aux_rh = ws.rh, .aux_h = ws.hx, .ldh = HX_LD});
            L.conv(C(q), {.in0 = ws.rh, .ld0 = HD, .c0 = HD, .in1 = ws.hx + MOT_OFF, .ld1 = HX_LD, .c1 = 128, .B = B, .Hin = h, .Win = w,
                          .epi = OFX_EPI_GRU_Q, .addend = g + 2 * HD, .ldadd = GADD_LD, .aux_z = ws.z, .aux_h = ws.hx, .ldh = HX_LD});
        }
        // flow head (update.py:6-14) + coords1 += delta (raft.py:131) in the epilogue
        L.conv(C("fh1"), {.in0 = ws.hx, .ld0 = HX_LD, .c0 = HD, .out = ws.c1, .ldo = 256, .B = B, .Hin = h, .Win = w, .act = OFX_ACT_RELU});
        if (!L.st) {   // 256 -> 2 channels: dedicated reduction kernel instead of a 1/16-utilised GEMM tile
            const ConvW& f2 = C("fh2");
            const hipEvent_t fork_ev = it + 1 < iters ? S.arm_fork() : nullptr;
            L.st = ofx_flow_head_launch(ws.c1, 256, f2.w, (int)f2.kpad, f2.shift, ws.coords1, ws.hx + FLOW_OFF, HX_LD, ws.frows, B, h,
                                        w, s, fork_ev);
            fork_on_kernel = fork_ev && !L.st;   // the flow head has one launch: it took the event unless the call failed
        }
    }
    // mask head (update.py:122-125,135) on the final hidden state
    L.conv(C("mask0"), {.in0 = ws.hx, .ld0 = HX_LD, .c0 = HD, .out = ws.c1, .ldo = 256, .B = B, .Hin = h, .Win = w, .act = OFX_ACT_RELU});
    L.conv(C("mask2"), {.in0 = ws.c1, .ld0 = 256, .c0 = 256, .out = ws.mask, .ldo = 576, .B = B, .Hin = h, .Win = w});
    return L.st;
}

// The volume GEMM on the A-stationary kernel (corr_split.hip).  OFX_RAFT_VOL_BF16X3 / _BF16X6 ask for its split-bf16 forms alone (every
// convolution stays fp32), the all-layer split modes take them along.  Its operands in fragment order live in the recurrence's scratch
// (corr ... mask: dead until the first iteration).  0 = the generic batched GEMM of conv.hip (shapes the kernel does not take).
static int volume_planes(const Call& c, const RaftWs& ws) {
    if (c.alt) return 0;
    const int flags = c.flags, h = c.h, w = c.w;
    // 1: the exact-fp32 form of the same A-stationary kernel (round 6: bit-identical to the generic batched GEMM it replaces, whole-line
    // stores, no operand re-fetch) -- the default wherever the shape allows; OFX_VOL_GENERIC=1 keeps the generic GEMM (diagnostic)
    const int planes = (flags & (OFX_RAFT_VOL_BF16X6 | OFX_RAFT_BF16X6)) ? 3 : (flags & (OFX_RAFT_VOL_BF16X3 | OFX_RAFT_BF16X3)) ? 2 : 1;
    static const bool generic = getenv("OFX_VOL_GENERIC") != nullptr;
    if ((planes == 1 && generic) || !ofx_corr_volsplit_ok(h, w, FD) || !ofx_corr_volsplit_pays(c.B, h, w, planes) || getenv("OFX_NO_VOLSPLIT")) return 0;
    const size_t room = (size_t)((const char*)(ws.mask + c.M * 576) - (const char*)ws.corr);
    return (size_t)((long)c.n1 + c.n2) * ofx_corr_planes_bytes(h, w, planes) <= room ? planes : 0;
}

// the workspace of a parsed call, its split-K arrival counters at zero (the kernels leave them at zero)
static int open_workspace(RaftWs* ws, const Call& c) {
    *ws = carve(c.workspace, c.workspace_bytes, c.B, c.H, c.W, c.flags, c.n_images);
    OFX_REQUIRE(ws->bytes <= c.workspace_bytes, OFX_ENOMEM);
    for (int e = 0; e < 3; ++e)
        if (ws->sk[e]) OFX_HIP_CHECK(hipMemsetAsync(ws->sk[e], 0, 65536, c.s));
    return 0;
}

static int basic_forward(ofx_raft* r, const Call& c) {
    RaftWs ws;
    int st = open_workspace(&ws, c);
    if (st) return st;
    const uint8_t *image1 = c.image1, *image2 = c.image2;
    const int B = c.B, H = c.H, W = c.W, n1 = c.n1, n2 = c.n2, bgr = c.bgr, prec = c.prec;
    const long N = c.N, M = c.M;
    const bool sh1 = c.sh1, sh2 = c.sh2, bnb = c.bnb, sepst = c.sepst;
    hipStream_t s = c.s;
    const long img_bytes = (long)H * W * 3;
    const char* cnet = bnb ? "cnetb" : "cnet";

    // ---- encoders (instance norm => per-image statistics, so chunking is exact).  Three independent chains:
    // fnet(image1) on the caller's stream, fnet(image2) and cnet(image1) on the side streams when the batch is
    // too small to fill the machine by itself.
    const bool overlap = overlap_pays(M) && !c.serial;
    const Streams S{r, s, overlap};
    const int ech = enc_chunk(H, W);
    if ((st = S.fork(0))) return st;
    if ((st = S.fork(1))) return st;
    // A shared key frame encoded by itself is a single-image launch sequence on a 256-CU part (1.3 ms where 1/64 of the frames' pass is
    // 0.3): large batches append it to the last chunk of the frames instead -- instance norm is per image, so the result is the same
    // network; its feature map lands right behind the frames' (fmap2 follows fmap1 in the workspace).
    const long half_bytes = (long)(H / 2) * (W / 2) * 64 * 4;
    const bool fold_key = sh2 && !sh1 && !overlap_pays(M) && ws.fmap2 == ws.fmap1 + (long)n1 * N * FD &&   // (by batch size, not by schedule: OFX_RAFT_SERIAL must not change the arithmetic)
                          (long)(std::min(ech, (n1 - 1) % ech + 1) + 1) * half_bytes < (1L << 31) - 4096;
    for (int i0 = 0; i0 < n1 && !st; i0 += ech) {
        const int n = std::min(ech, n1 - i0);
        const bool last = i0 + n == n1;
        st = run_encoder(r, "fnet", false, image1 + i0 * img_bytes, n, H, W, bgr, ws.eb[0], ws.fmap1 + (long)i0 * N * FD, FD,
                         false, 0, s, prec, sepst, (fold_key && last) ? image2 : nullptr);
    }
    for (int i0 = 0; i0 < n2 && !st && !fold_key; i0 += ech) {
        const int n = std::min(ech, n2 - i0);
        st = run_encoder(r, "fnet", false, image2 + i0 * img_bytes, n, H, W, bgr, ws.eb[1], ws.fmap2 + (long)i0 * N * FD, FD,
                         false, 0, S.get(0), prec, sepst);
    }
    // context encoder on image1 -> hx[:, 0:128] = tanh (net), hx[:, 256:384] = relu (inp)
    if (sh1) {
        if (!st) st = run_encoder(r, cnet, !bnb, image1, 1, H, W, bgr, ws.eb[2], ws.hx, HX_LD, true, INP_OFF, S.get(1), prec, sepst);
        for (int k = 1; k < B && !st; ++k)   // one shared image1: replicate its context rows
            OFX_HIP_CHECK(hipMemcpyAsync(ws.hx + (long)k * N * HX_LD, ws.hx, (size_t)N * HX_LD * sizeof(float),
                                         hipMemcpyDeviceToDevice, S.get(1)));
    } else {
        for (int i0 = 0; i0 < B && !st; i0 += ech) {
            const int n = std::min(ech, B - i0);
            st = run_encoder(r, cnet, !bnb, image1 + i0 * img_bytes, n, H, W, bgr, ws.eb[2], ws.hx + (long)i0 * N * HX_LD,
                             HX_LD, true, INP_OFF, S.get(1), prec, sepst);
        }
    }
    if (!st) st = S.join(0);
    if (!st) st = S.join(1);
    if (st) return st;

    // ---- correlation; the split planes live in the recurrence's scratch (volume_planes)
    PairMap pm;
    if ((st = make_pair_map(&pm, c, ws.idx_dev, c.alt, c.alt))) return st;
    st = correlate(c, ws, pm, FD, prec, volume_planes(c, ws), ws.corr);
    if (!st && c.warped) st = ofx_warp_pad_launch(c.warp_frame, ws.warp_pad, H, W, s);   // the zero-bordered RGBX copy the warp samples (1.6 MB at 512x768: stays in L2)
    if (!st) st = run_recurrence(r, ws, c, pm, overlap);
    if (!st) st = finish_flow(c, ws.coords1, ws.mask, ws.warp_pad);
    if (st) return st;
    register_buffers(r, c, ws, FD, ws.hx, HX_LD, ws.coords1, ws.corr, CORR_LD, ws.mask);   // corr rows of 336: 324 features + 12 zeros
    return 0;
}

static int basic_forward_pairs(ofx_raft* r, const Call& c) {
    RaftWs ws;
    int st = open_workspace(&ws, c);
    if (st) return st;
    const uint8_t* images = c.image1;
    const int n_images = c.n_images, B = c.B, H = c.H, W = c.W, bgr = c.bgr, prec = c.prec;
    const long N = c.N;
    const bool bnb = c.bnb, sepst = c.sepst;
    hipStream_t s = c.s;
    const long img_bytes = (long)H * W * 3;
    const char* cnet = bnb ? "cnetb" : "cnet";
    // every image is encoded ONCE (feature + context), however many pairs it takes part in: a 15-frame
    // KeyframeConv window has 210 ordered pairs but only 15 images (ofgen_keyframe_inpaint.py:627-668)
    const bool overlap = overlap_pays(c.M) && !c.serial;
    const Streams S{r, s, overlap};
    if ((st = S.fork(1))) return st;
    for (int i0 = 0; i0 < n_images && !st; i0 += enc_chunk(H, W)) {
        const int n = std::min(enc_chunk(H, W), n_images - i0);
        st = run_encoder(r, "fnet", false, images + i0 * img_bytes, n, H, W, bgr, ws.eb[0], ws.fmap1 + (long)i0 * N * FD, FD,
                         false, 0, s, prec, sepst);
        if (!st)
            st = run_encoder(r, cnet, !bnb, images + i0 * img_bytes, n, H, W, bgr, ws.eb[2], ws.ctx + (long)i0 * N * (HD + CD),
                             HD + CD, true, HD, S.get(1), prec, sepst);
    }
    if (!st) st = S.join(1);
    if (st) return st;
    // the pair list on the device: image1's for the context rows, image2's too where the lookup or the split-plane volume reads it
    const int vplanes = volume_planes(c, ws);
    PairMap pm;
    if ((st = make_pair_map(&pm, c, ws.idx_dev, true, c.alt || vplanes))) return st;
    st = ofx_ctx_gather(ws.ctx, pm.d1, ws.hx, HX_LD, INP_OFF, HD, B, N, s);
    if (!st) st = correlate(c, ws, pm, FD, prec, vplanes, ws.corr);
    if (!st && c.warped) st = ofx_warp_pad_launch(c.warp_frame, ws.warp_pad, H, W, s);   // the zero-bordered RGBX copy the warp samples
    if (!st) st = run_recurrence(r, ws, c, pm, overlap);
    if (!st) st = finish_flow(c, ws.coords1, ws.mask, ws.warp_pad);
    if (st) return st;
    r->bufs.clear();   // the indexed-pairs call registers nothing
    return 0;
}

// ============================================================================================
// The small network (raft-small.pth; RAFT/core/raft.py:29-33, :48-51): SmallEncoder feature / context networks
// (extractor.py:195-267, bottleneck blocks :60-116), radius-3 lookup, SmallUpdateBlock (update.py:62-77, :99-112: a 3x3 ConvGRU,
// no mask head) and upflow8 (utils/utils.py:80-82) in place of the convex upsample.  Everything runs on the general kernels the
// basic network's schedule also uses (ofx_conv2d, ofx_inorm_*, the blocked volume + pool, ofx_corr_lookup's generic kernel,
// ofx_local_corr) plus ofx_upflow8 / its warp form; every launch stays on the caller's stream (no side streams, no stop events).
//
//   encoders   preprocess -> 7x7/s2 conv (3 -> 32) -> 3 stages x 2 bottleneck blocks (32, 64, 96) -> 1x1 conv
//              fnet: InstanceNorm2d without affine -- statistics pass + normalise/ReLU pass after each raw convolution;
//              cnet: no norm at all -- ReLU and the residual add live in the convolution epilogues
//   volume     D = 128 (scaled by 1 / sqrt(128)); the same batched GEMM + pooling kernels as the basic network
//   iteration  lookup (4 x 49) -> convc1 -> convf1 -> convf2 -> conv -> zr -> q -> flow head (EPI_FLOW: coords1 += delta)
//   tail       upflow8 (optionally with the warp of one shared frame) of the last iteration only
namespace {

constexpr int S_HD = 96, S_CD = 64, S_FD = 128, S_RADIUS = 3;
constexpr int S_CORR_CH = LEVELS * (2 * S_RADIUS + 1) * (2 * S_RADIUS + 1);   // 196
// convc1's operand row: 196 correlation features + 28 zeros (Kpad of a 1x1 conv over 196 channels is 224 anyway).  The generic
// lookup writes only the features: the zeros are set once per forward (a NaN left in them times a zero weight would be NaN).
constexpr int S_CORR_LD = 224;
// hx row = [h(96) | inp(64) | motion(80) flow(2) | 14 zeros] = 256: the ConvGRU's cat([h, x]) (update.py:20-21) with
// x = cat([inp, motion features]) (update.py:109); the zeros make x a whole number of 32-channel K chunks for the q convolution's
// second segment (cat([r*h, x]), update.py:26).  The zeros are set once per forward.
constexpr int S_HX_LD = 256, S_INP_OFF = S_HD, S_MOT_OFF = S_HD + S_CD, S_FLOW_OFF = S_MOT_OFF + 80;
constexpr int S_X_CH = S_HX_LD - S_HD;   // 160

struct SmallWs : CorrWs {
    float *x0, *X, *Y, *T1, *T2, *T3, *Dn, *N1, *N2;   // encoder activations of one chunk
    float* stats;      // 8 x [chunk][128]: mean / rstd of up to four norms
    float* scratch;    // f64 partial sums of ofx_inorm_stats
    float* ctx;
    float *hx, *coords1, *flow4, *corr, *corflo, *f1, *z, *rh, *fh;
    int nch;
    size_t bytes;
};

SmallWs small_carve(void* base, size_t cap, int B, int H, int W, int flags, int n_images) {
    SmallWs w{};
    Carver c(base, cap);
    const int h = H / 8, wd = W / 8;
    const long N = (long)h * wd, M = (long)B * N;
    const int most = n_images > 0 ? n_images : std::max(B, 1);
    w.nch = std::min(enc_chunk(H, W), most);
    const size_t act = (size_t)w.nch * (H / 2) * (W / 2) * 32;   // the widest activation: 32 channels at half resolution
    w.x0 = c.take((size_t)w.nch * H * W * 4);
    float** bufs[8] = {&w.X, &w.Y, &w.T1, &w.T2, &w.T3, &w.Dn, &w.N1, &w.N2};
    for (float** b : bufs) *b = c.take(act);
    w.stats = c.take((size_t)8 * w.nch * 128);
    w.scratch = c.take((size_t)std::max(w.nch * 64, std::min(w.nch, 7) * 256) * 128 * 2 * 2);   // doubles (ofx.h: ofx_inorm_stats)
    long n1 = (flags & OFX_RAFT_SHARED_IMG1) ? 1 : B, n2 = (flags & OFX_RAFT_SHARED_IMG2) ? 1 : B;
    if (n_images > 0) {
        n1 = n_images;
        n2 = 0;
        w.ctx = c.take((size_t)n_images * N * S_HX_LD);
    }
    // index slots, volume-free mode only: image indices per pair (image1's, then image2's) for the tiled lookup
    const bool alt = flags & OFX_RAFT_ALT_CORR;
    carve_corr(&w, c, S_FD, B, H, W, n1, n2, n_images, alt, alt ? 2 * B : 0);
    w.hx = c.take((size_t)M * S_HX_LD);
    w.coords1 = c.take((size_t)M * 2);
    w.flow4 = c.take((size_t)M * FROW);   // [M][4] flow operand of convf1 (EPI_FLOW); 16 floats a pixel: ofx_init_state zeroes that many
    w.corr = c.take((size_t)M * S_CORR_LD);
    w.corflo = c.take((size_t)M * 128);
    w.f1 = c.take((size_t)M * 64);
    w.z = c.take((size_t)M * S_HD);
    w.rh = c.take((size_t)M * S_HD);
    w.fh = c.take((size_t)M * 128);
    w.bytes = c.off;
    return w;
}

// one SmallEncoder over n images (u8 [n][H][W][3]); out [n*h*w][out_ld].  instance: fnet ('instance', no affine), else cnet ('none');
// tanh_rows > 0 (cnet): out rows [0, tanh_rows) = tanh, the rest = relu (raft.py:111-114)
int small_encoder(ofx_raft* r, const char* enc, bool instance, const uint8_t* imgs, int n, int H, int W, int bgr, const SmallWs& ws, float* out,
                  int out_ld, int tanh_rows, hipStream_t s) {
    Launcher L(s);
    auto C = [&](const std::string& k) -> const ConvW& { return r->convs[std::string(enc) + "." + k]; };
    const int SC = ws.nch * 128;
    float* mean[4] = {ws.stats, ws.stats + 2 * SC, ws.stats + 4 * SC, ws.stats + 6 * SC};
    float* rstd[4] = {ws.stats + SC, ws.stats + 3 * SC, ws.stats + 5 * SC, ws.stats + 7 * SC};
    auto stats = [&](const float* x, long HW, int ch, int k) {
        if (!L.st) L.st = ofx_inorm_stats(x, ch, mean[k], rstd[k], ws.scratch, n, HW, ch, 1e-5f, s);
    };
    auto norm_relu = [&](const float* x, long HW, int ch, int k, float* o) {   // o = relu(inorm(x))
        if (!L.st) L.st = ofx_inorm_apply(x, mean[k], rstd[k], nullptr, nullptr, nullptr, o, n, HW, ch, 1, s);
    };
    int st = ofx_preprocess_u8(imgs, ws.x0, (long)n * H * W, bgr, s);
    if (st) return st;
    float* X = ws.X;
    float* Y = ws.Y;
    int hin = H / 2, win = W / 2, cin = 32;
    if (instance) {
        L.conv(C("conv1"), {.in0 = ws.x0, .ld0 = 4, .c0 = 4, .out = ws.T3, .ldo = 32, .B = n, .Hin = H, .Win = W, .stride = 2});
        stats(ws.T3, (long)hin * win, 32, 0);
        norm_relu(ws.T3, (long)hin * win, 32, 0, X);
    } else {
        L.conv(C("conv1"), {.in0 = ws.x0, .ld0 = 4, .c0 = 4, .out = X, .ldo = 32, .B = n, .Hin = H, .Win = W, .stride = 2, .act = OFX_ACT_RELU});
    }
    const int dims[3] = {32, 64, 96};
    for (int li = 1; li <= 3; ++li) {
        const int dim = dims[li - 1], mid = dim / 4;
        for (int bi = 0; bi < 2; ++bi) {
            const int stride = (li > 1 && bi == 0) ? 2 : 1;
            const int ho = (hin - 1) / stride + 1, wo = (win - 1) / stride + 1;   // 3x3 pad 1 and 1x1 pad 0: the same output size
            const long HWo = (long)ho * wo;
            const std::string p = "layer" + std::to_string(li) + "." + std::to_string(bi);
            if (instance) {
                L.conv(C(p + ".conv1"), {.in0 = X, .ld0 = cin, .c0 = cin, .out = ws.T1, .ldo = mid, .B = n, .Hin = hin, .Win = win});
                stats(ws.T1, (long)hin * win, mid, 0);
                norm_relu(ws.T1, (long)hin * win, mid, 0, ws.N1);
                L.conv(C(p + ".conv2"), {.in0 = ws.N1, .ld0 = mid, .c0 = mid, .out = ws.T2, .ldo = mid, .B = n, .Hin = hin, .Win = win, .stride = stride});
                stats(ws.T2, HWo, mid, 1);
                norm_relu(ws.T2, HWo, mid, 1, ws.N2);
                L.conv(C(p + ".conv3"), {.in0 = ws.N2, .ld0 = mid, .c0 = mid, .out = ws.T3, .ldo = dim, .B = n, .Hin = ho, .Win = wo});
                stats(ws.T3, HWo, dim, 2);
                if (stride == 2) {   // relu(norm4(down(x)) + relu(norm3(conv3)))
                    L.conv(C(p + ".down"), {.in0 = X, .ld0 = cin, .c0 = cin, .out = ws.Dn, .ldo = dim, .B = n, .Hin = hin, .Win = win, .stride = 2});
                    stats(ws.Dn, HWo, dim, 3);
                    if (!L.st) L.st = ofx_inorm_apply(ws.T3, mean[2], rstd[2], ws.Dn, mean[3], rstd[3], Y, n, HWo, dim, 1, s);
                } else {             // relu(x + relu(norm3(conv3)))
                    if (!L.st) L.st = ofx_inorm_apply(ws.T3, mean[2], rstd[2], X, nullptr, nullptr, Y, n, HWo, dim, 1, s);
                }
            } else {
                L.conv(C(p + ".conv1"), {.in0 = X, .ld0 = cin, .c0 = cin, .out = ws.T1, .ldo = mid, .B = n, .Hin = hin, .Win = win, .act = OFX_ACT_RELU});
                L.conv(C(p + ".conv2"), {.in0 = ws.T1, .ld0 = mid, .c0 = mid, .out = ws.T2, .ldo = mid, .B = n, .Hin = hin, .Win = win, .stride = stride,
                                         .act = OFX_ACT_RELU});
                const float* res = X;
                if (stride == 2) {
                    L.conv(C(p + ".down"), {.in0 = X, .ld0 = cin, .c0 = cin, .out = ws.Dn, .ldo = dim, .B = n, .Hin = hin, .Win = win, .stride = 2});
                    res = ws.Dn;
                }
                // relu(x' + relu(conv3)): the residual merge of EPI_PLAIN
                L.conv(C(p + ".conv3"), {.in0 = ws.T2, .ld0 = mid, .c0 = mid, .out = Y, .ldo = dim, .B = n, .Hin = ho, .Win = wo, .act = OFX_ACT_RELU,
                                         .res = res, .ldres = dim});
            }
            std::swap(X, Y);
            hin = ho; win = wo; cin = dim;
        }
    }
    const ConvArgs last{.in0 = X, .ld0 = 96, .c0 = 96, .out = out, .ldo = out_ld, .B = n, .Hin = hin, .Win = win};
    if (tanh_rows <= 0) L.conv(C("conv2"), last);
    else L.conv_tanh_relu(C("conv2"), last, tanh_rows, tanh_rows);
    return L.st;
}

// state init, `iters` refinement iterations of SmallUpdateBlock (upflow8 of the last iteration only -- raft.py:134-135; test_mode returns
// the last prediction -- is finish_flow's)
// (c.warm: flow_low holds the initial flow, OFX_RAFT_FLOW_INIT)
int small_recurrence(ofx_raft* r, const SmallWs& ws, const Call& c, const PairMap& aix) {
    const int B = c.B, h = c.h, w = c.w, iters = c.iters;
    const bool alt = c.alt;
    hipStream_t s = c.s;
    const long M = c.M;
    int st = c.warm ? ofx_init_state_warm(ws.coords1, ws.flow4, ws.hx, S_HX_LD, S_FLOW_OFF, true, c.flow_low, B, h, w, s)
                  : ofx_init_state(ws.coords1, ws.flow4, ws.hx, S_HX_LD, S_FLOW_OFF, B, h, w, s);
    if (st) return st;
    OFX_HIP_CHECK(hipMemsetAsync(ws.corr, 0, (size_t)M * S_CORR_LD * sizeof(float), s));   // the 28 pad columns of every row
    Launcher L(s);
    auto C = [&](const char* k) -> const ConvW& { return r->convs[k]; };
    const float* pyr_c[LEVELS] = {ws.pyr[0], ws.pyr[1], ws.pyr[2], ws.pyr[3]};
    for (int it = 0; it < iters && !L.st; ++it) {
        if (!alt) {
            L.st = ofx_corr_lookup(pyr_c, ws.coords1, ws.corr, S_CORR_LD, B, h, w, LEVELS, S_RADIUS, s);
        } else {
            L.st = alt_lookup(ws.fmap1, ws.f2l, aix, ws.coords1, ws.corr, S_CORR_LD, B, h, w, S_FD, S_RADIUS, s);
        }
        // SmallMotionEncoder (update.py:70-77): cor_flo = [relu(convc1(corr)) (96) | relu(convf2(relu(convf1(flow)))) (32)]
        L.conv(C("convc1"), {.in0 = ws.corr, .ld0 = S_CORR_LD, .c0 = S_CORR_LD, .out = ws.corflo, .ldo = 128, .B = B, .Hin = h, .Win = w,
                             .act = OFX_ACT_RELU});
        L.conv(C("convf1"), {.in0 = ws.flow4, .ld0 = 4, .c0 = 4, .out = ws.f1, .ldo = 64, .B = B, .Hin = h, .Win = w, .act = OFX_ACT_RELU});
        L.conv(C("convf2"), {.in0 = ws.f1, .ld0 = 64, .c0 = 64, .out = ws.corflo + 96, .ldo = 128, .B = B, .Hin = h, .Win = w, .act = OFX_ACT_RELU});
        L.conv(C("conv"), {.in0 = ws.corflo, .ld0 = 128, .c0 = 128, .out = ws.hx + S_MOT_OFF, .ldo = S_HX_LD, .B = B, .Hin = h, .Win = w,
                           .act = OFX_ACT_RELU});
        // ConvGRU (update.py:16-31): z | r in one convolution over cat([h, x]), q over cat([r*h, x]), h updated in place
        L.conv(C("gru.zr"), {.in0 = ws.hx, .ld0 = S_HX_LD, .c0 = S_HX_LD, .B = B, .Hin = h, .Win = w, .epi = OFX_EPI_GRU_ZR, .aux_z = ws.z,
                             .aux_rh = ws.rh, .aux_h = ws.hx, .ldh = S_HX_LD});
        L.conv(C("gru.q"), {.in0 = ws.rh, .ld0 = S_HD, .c0 = S_HD, .in1 = ws.hx + S_INP_OFF, .ld1 = S_HX_LD, .c1 = S_X_CH, .B = B, .Hin = h,
                            .Win = w, .epi = OFX_EPI_GRU_Q, .aux_z = ws.z, .aux_h = ws.hx, .ldh = S_HX_LD});
        // FlowHead(96, 128) (update.py:6-14); coords1 += delta in the second convolution's epilogue (one rounding: delta, then the add),
        // which also leaves the new flow in hx's flow slot and in convf1's operand
        L.conv(C("fh1"), {.in0 = ws.hx, .ld0 = S_HX_LD, .c0 = S_HD, .out = ws.fh, .ldo = 128, .B = B, .Hin = h, .Win = w, .act = OFX_ACT_RELU});
        L.conv(C("fh2"), {.in0 = ws.fh, .ld0 = 128, .c0 = 128, .B = B, .Hin = h, .Win = w, .epi = OFX_EPI_FLOW, .aux_h = ws.hx + S_FLOW_OFF,
                          .ldh = S_HX_LD, .aux_coords = ws.coords1, .aux_flow4 = ws.flow4});
    }
    return L.st;
}

// the split-bf16 modes have no small-network form: its convolutions and its D = 128 volume run in exact fp32 only
constexpr int S_UNSUPPORTED = OFX_RAFT_BF16X3 | OFX_RAFT_BF16X6 | OFX_RAFT_VOL_BF16X3 | OFX_RAFT_VOL_BF16X6 | OFX_RAFT_F16;

}  // namespace

// 0 = basic, 1 = small, OFX_EKEY = neither, or keys of both
static int small_detect(const std::map<std::string, HostTensor>& sd) {
    auto has = [&](const char* k) { return sd.count(k) > 0; };
    const bool small = has("update_block.gru.convz.weight") && has("fnet.layer1.0.conv3.weight");
    const bool basic_marks = has("update_block.gru.convz1.weight") || has("update_block.mask.0.weight") ||
                             has("update_block.encoder.convc2.weight") || has("cnet.norm1.weight");
    const bool small_marks = has("update_block.gru.convz.weight") || has("fnet.layer1.0.conv3.weight") || has("cnet.layer1.0.conv3.weight");
    if (small && !basic_marks) return 1;
    if (small_marks) return OFX_EKEY;
    return 0;
}

static int small_build(ofx_raft* r, const std::map<std::string, HostTensor>& sd) {
    for (const char* enc : {"fnet", "cnet"}) {
        const std::string e = enc;
        int st = add_conv(r, sd, e + ".conv1", e + ".conv1", 4, "", 1.f);
        if (st) return st;
        for (int li = 1; li <= 3; ++li)
            for (int bi = 0; bi < 2; ++bi) {
                const std::string p = e + ".layer" + std::to_string(li) + "." + std::to_string(bi);
                for (const char* cv : {".conv1", ".conv2", ".conv3"}) {
                    st = add_conv(r, sd, p + cv, p + cv, 0, "", 1.f);
                    if (st) return st;
                }
                if (li > 1 && bi == 0) {
                    st = add_conv(r, sd, p + ".downsample.0", p + ".down", 0, "", 1.f);
                    if (st) return st;
                }
            }
        st = add_conv(r, sd, e + ".conv2", e + ".conv2", 0, "", 1.f);
        if (st) return st;
    }
    const ConvW& fo = r->convs["fnet.conv2"];
    const ConvW& co = r->convs["cnet.conv2"];
    if (fo.cout != S_FD || fo.cin != 96 || co.cout != S_HD + S_CD || co.cin != 96) return OFX_EKEY;
    const std::string ub = "update_block.";
    int st = add_conv(r, sd, ub + "encoder.convc1", "convc1", S_CORR_LD, "", 1.f);
    if (!st && (r->convs["convc1"].cin != S_CORR_CH || r->convs["convc1"].cout != 96)) st = OFX_EKEY;
    if (!st) st = add_conv(r, sd, ub + "encoder.convf1", "convf1", 4, "", 1.f);   // 7x7 over the [M][4] flow operand (channels 2, 3 zero)
    if (!st) st = add_conv(r, sd, ub + "encoder.convf2", "convf2", 0, "", 1.f);
    if (!st) st = add_conv(r, sd, ub + "encoder.conv", "conv", 0, "", 1.f);
    if (!st && (r->convs["conv"].cout != 80 || r->convs["convf2"].cout != 32)) st = OFX_EKEY;
    if (!st) {   // z and r share their input: one convolution with Cout = 192 ([convz ; convr] rows), input rows padded 242 -> 256
        std::vector<float> wzr, shzr;
        st = add_conv(r, sd, ub + "gru.convz", "gru.z", S_HX_LD, "", 1.f, &wzr, &shzr);
        if (!st) st = add_conv(r, sd, ub + "gru.convr", "gru.r", S_HX_LD, "", 1.f, &wzr, &shzr);
        if (!st) {
            ConvW c = r->convs["gru.z"];
            if (c.cout != S_HD || c.cin != S_HX_LD - 14 || c.kh != 3 || c.kw != 3) return OFX_EKEY;
            c.cout *= 2;
            st = upload_weight(r, wzr, &c);
            if (!st) st = upload(r, shzr, &c.shift);
            c.name = "gru.zr";
            r->convs["gru.zr"] = c;
        }
    }
    if (!st) st = add_conv(r, sd, ub + "gru.convq", "gru.q", S_HX_LD, "", 1.f);
    if (!st) st = add_conv(r, sd, ub + "flow_head.conv1", "fh1", 0, "", 1.f);
    if (!st) st = add_conv(r, sd, ub + "flow_head.conv2", "fh2", 0, "", 1.f);
    if (!st && (r->convs["fh1"].cin != S_HD || r->convs["fh2"].cout != 2)) st = OFX_EKEY;
    return st;
}

static size_t small_workspace_bytes(int B, int H, int W, int n_images) {
    if (n_images > 0) return small_carve(nullptr, 0, B, H, W, 0, n_images).bytes;
    const size_t a = small_carve(nullptr, 0, B, H, W, 0, 0).bytes, b = small_carve(nullptr, 0, B, H, W, OFX_RAFT_ALT_CORR, 0).bytes;
    return a > b ? a : b;
}

static size_t small_workspace_bytes_mode(int B, int H, int W, int flags, int n_images) { return small_carve(nullptr, 0, B, H, W, flags, n_images).bytes; }

static int small_forward(ofx_raft* r, const Call& c) {
    const SmallWs ws = small_carve(c.workspace, c.workspace_bytes, c.B, c.H, c.W, c.flags, 0);
    OFX_REQUIRE(ws.bytes <= c.workspace_bytes, OFX_ENOMEM);
    const uint8_t *image1 = c.image1, *image2 = c.image2;
    const int B = c.B, H = c.H, W = c.W, n1 = c.n1, n2 = c.n2, bgr = c.bgr;
    const long N = c.N, M = c.M, img_bytes = (long)H * W * 3;
    hipStream_t s = c.s;
    int st = 0;
    OFX_HIP_CHECK(hipMemsetAsync(ws.hx, 0, (size_t)M * S_HX_LD * sizeof(float), s));   // the 14 pad columns of every row
    for (int i0 = 0; i0 < n1 && !st; i0 += ws.nch)
        st = small_encoder(r, "fnet", true, image1 + i0 * img_bytes, std::min(ws.nch, n1 - i0), H, W, bgr, ws, ws.fmap1 + (long)i0 * N * S_FD, S_FD,
                           0, s);
    for (int i0 = 0; i0 < n2 && !st; i0 += ws.nch)
        st = small_encoder(r, "fnet", true, image2 + i0 * img_bytes, std::min(ws.nch, n2 - i0), H, W, bgr, ws, ws.fmap2 + (long)i0 * N * S_FD, S_FD,
                           0, s);
    // context network on image1 -> hx[:, 0:96] = tanh (net), hx[:, 96:160] = relu (inp)
    for (int i0 = 0; i0 < n1 && !st; i0 += ws.nch)
        st = small_encoder(r, "cnet", false, image1 + i0 * img_bytes, std::min(ws.nch, n1 - i0), H, W, bgr, ws, ws.hx + (long)i0 * N * S_HX_LD,
                           S_HX_LD, S_HD, s);
    for (int k = 1; k < B && !st && c.sh1; ++k)   // one shared image1: replicate its context rows
        OFX_HIP_CHECK(hipMemcpyAsync(ws.hx + (long)k * N * S_HX_LD, ws.hx, (size_t)N * S_HX_LD * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (st) return st;
    PairMap pm;
    if ((st = make_pair_map(&pm, c, ws.idx_dev, c.alt, c.alt))) return st;
    st = correlate(c, ws, pm, S_FD, OFX_PREC_FP32, 0, nullptr);
    if (!st && c.warped) st = ofx_warp_pad_launch(c.warp_frame, ws.warp_pad, H, W, s);
    if (!st) st = small_recurrence(r, ws, c, pm);
    if (!st) st = finish_flow(c, ws.coords1, nullptr, ws.warp_pad);   // no mask head: upflow8
    if (st) return st;
    // hx rows of 256: h (96) | inp (64) | motion (80) | flow (2) | zeros; corr rows of 224: 196 features + 28 zeros
    register_buffers(r, c, ws, S_FD, ws.hx, S_HX_LD, ws.coords1, ws.corr, S_CORR_LD, nullptr);
    return 0;
}

static int small_forward_pairs(ofx_raft* r, const Call& c) {
    const SmallWs ws = small_carve(c.workspace, c.workspace_bytes, c.B, c.H, c.W, c.flags, c.n_images);
    OFX_REQUIRE(ws.bytes <= c.workspace_bytes, OFX_ENOMEM);
    const uint8_t* images = c.image1;
    const int* idx1 = c.idx1;
    const int n_images = c.n_images, B = c.B, H = c.H, W = c.W, bgr = c.bgr;
    const long N = c.N, img_bytes = (long)H * W * 3;
    hipStream_t s = c.s;
    int st = 0;
    // every image is encoded once (feature + context network), however many pairs it takes part in; its context rows are laid out as
    // the hx rows they are copied into (pad columns zero)
    OFX_HIP_CHECK(hipMemsetAsync(ws.ctx, 0, (size_t)n_images * N * S_HX_LD * sizeof(float), s));
    for (int i0 = 0; i0 < n_images && !st; i0 += ws.nch) {
        const int n = std::min(ws.nch, n_images - i0);
        st = small_encoder(r, "fnet", true, images + i0 * img_bytes, n, H, W, bgr, ws, ws.fmap1 + (long)i0 * N * S_FD, S_FD, 0, s);
        if (!st) st = small_encoder(r, "cnet", false, images + i0 * img_bytes, n, H, W, bgr, ws, ws.ctx + (long)i0 * N * S_HX_LD, S_HX_LD, S_HD, s);
    }
    for (int b = 0; b < B && !st; ++b)
        OFX_HIP_CHECK(hipMemcpyAsync(ws.hx + (long)b * N * S_HX_LD, ws.ctx + (long)idx1[b] * N * S_HX_LD, (size_t)N * S_HX_LD * sizeof(float),
                                     hipMemcpyDeviceToDevice, s));
    if (st) return st;
    PairMap pm;   // volume-free: the pair list on the device for the lookup
    if ((st = make_pair_map(&pm, c, ws.idx_dev, c.alt, c.alt))) return st;
    st = correlate(c, ws, pm, S_FD, OFX_PREC_FP32, 0, nullptr);
    if (!st && c.warped) st = ofx_warp_pad_launch(c.warp_frame, ws.warp_pad, H, W, s);
    if (!st) st = small_recurrence(r, ws, c, pm);
    if (!st) st = finish_flow(c, ws.coords1, nullptr, ws.warp_pad);
    if (st) return st;
    r->bufs.clear();   // the indexed-pairs call registers nothing
    return 0;
}

extern "C" {

int ofx_raft_create(const ofx_tensor* tensors, int n, ofx_raft** out) {
    OFX_REQUIRE(tensors && n > 0 && out, OFX_EINVAL);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return OFX_ENODEV;
    std::map<std::string, HostTensor> sd;
    for (int i = 0; i < n; ++i) {
        if (!tensors[i].name || !tensors[i].data) continue;
        std::string k = tensors[i].name;
        if (k.rfind("module.", 0) == 0) k = k.substr(7);
        HostTensor t;
        t.data = tensors[i].data;
        t.ndim = tensors[i].ndim;
        for (int j = 0; j < 4; ++j) t.shape[j] = j < t.ndim ? tensors[i].shape[j] : 1;
        sd[k] = t;
    }
    const int variant = small_detect(sd);
    if (variant < 0) return variant;
    ofx_raft* r = new ofx_raft();
    r->variant = variant;
    if (variant == 1) {
        int st = small_build(r, sd);
        if (st) {
            ofx_raft_destroy(r);
            return st;
        }
        *out = r;
        return 0;
    }
    int st = build_encoder(r, sd, "fnet", false);
    if (!st) st = build_encoder(r, sd, "cnet", true);
    if (!st) st = build_encoder(r, sd, "cnet", true, "cnetb");
    const char* ub = "update_block.";
    if (!st) st = add_conv(r, sd, std::string(ub) + "encoder.convc1", "convc1", CORR_LD, "", 1.f);   // input rows padded to 336 (zero weights)
    if (!st) st = add_conv(r, sd, std::string(ub) + "encoder.convc2", "convc2", 0, "", 1.f);
    if (!st) st = add_wino(r, sd, {std::string(ub) + "encoder.convc2"}, {}, "convc2", true);
    std::vector<float> wf1;   // must outlive add_conv below
    if (!st) {
        // convf1 (7x7 on the 2-channel flow, update.py:93) as a 7x1 convolution over the 16-float flow rows the flow head leaves
        // (flow_head.hip): row channel kx * 2 + c = tap kx of input channel c, channels 14 and 15 are zero.  K = 112 instead of 196.
        const HostTensor* wf = find(sd, std::string(ub) + "encoder.convf1.weight");
        const HostTensor* bf = find(sd, std::string(ub) + "encoder.convf1.bias");
        if (!wf || !bf || wf->ndim != 4 || wf->shape[1] != 2 || wf->shape[2] != 7 || wf->shape[3] != 7) st = OFX_EKEY;
        if (!st) {
            const int co = (int)wf->shape[0];
            wf1.assign((size_t)co * 14 * 7, 0.f);
            for (int o = 0; o < co; ++o)
                for (int c = 0; c < 2; ++c)
                    for (int ky = 0; ky < 7; ++ky)
                        for (int kx = 0; kx < 7; ++kx)
                            wf1[((size_t)o * 14 + kx * 2 + c) * 7 + ky] = wf->data[(((size_t)o * 2 + c) * 7 + ky) * 7 + kx];
            HostTensor t;
            t.data = wf1.data(); t.ndim = 4;
            t.shape[0] = co; t.shape[1] = 14; t.shape[2] = 7; t.shape[3] = 1;
            sd["convf1_rows.weight"] = t;
            sd["convf1_rows.bias"] = *bf;
            st = add_conv(r, sd, "convf1_rows", "convf1", FROW, "", 1.f);
        }
    }
    if (!st) st = add_conv(r, sd, std::string(ub) + "encoder.convf2", "convf2", 0, "", 1.f);
    if (!st) st = add_wino(r, sd, {std::string(ub) + "encoder.convf2"}, {}, "convf2", true);
    if (!st) st = add_conv(r, sd, std::string(ub) + "encoder.conv", "conv", 0, "", 1.f);
    if (!st) st = add_wino(r, sd, {std::string(ub) + "encoder.conv"}, {}, "conv", true);
    if (!st) st = build_gru(r, sd, "1");
    if (!st) st = build_gru(r, sd, "2");
    if (!st) st = add_conv(r, sd, std::string(ub) + "flow_head.conv1", "fh1", 0, "", 1.f);
    if (!st) st = add_wino(r, sd, {std::string(ub) + "flow_head.conv1"}, {}, "fh1", true);
    if (!st) st = add_conv(r, sd, std::string(ub) + "flow_head.conv2", "fh2", 0, "", 1.f);
    if (!st) st = add_conv(r, sd, std::string(ub) + "mask.0", "mask0", 0, "", 1.f);
    if (!st) st = add_wino(r, sd, {std::string(ub) + "mask.0"}, {}, "mask0", true);
    if (!st) st = add_conv(r, sd, std::string(ub) + "mask.2", "mask2", 0, "", 0.25f);
    for (int i = 0; i < 2 && !st; ++i) {
        if (hipStreamCreateWithFlags(&r->aux[i], hipStreamNonBlocking) != hipSuccess) st = OFX_ENODEV;
        if (!st && hipEventCreateWithFlags(&r->ev_join[i], hipEventDisableTiming) != hipSuccess) st = OFX_ENODEV;
    }
    if (!st && hipEventCreateWithFlags(&r->ev_fork, hipEventDisableTiming) != hipSuccess) st = OFX_ENODEV;
    if (st) {
        ofx_raft_destroy(r);
        return st;
    }
    *out = r;
    return 0;
}

int ofx_raft_destroy(ofx_raft* r) {
    if (!r) return 0;
    for (void* p : r->allocs) (void)hipFree(p);
    for (int i = 0; i < 2; ++i) {
        if (r->aux[i]) (void)hipStreamDestroy(r->aux[i]);
        if (r->ev_join[i]) (void)hipEventDestroy(r->ev_join[i]);
    }
    if (r->ev_fork) (void)hipEventDestroy(r->ev_fork);
    delete r;
    return 0;
}

size_t ofx_raft_workspace_bytes(const ofx_raft* r, int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || (H % 8) || (W % 8)) return 0;
    if (r && r->variant == 1) return small_workspace_bytes(B, H, W, 0);
    // the volume layout is the larger of the two correlation modes
    size_t a = carve(nullptr, 0, B, H, W, 0).bytes;
    size_t b = carve(nullptr, 0, B, H, W, OFX_RAFT_ALT_CORR).bytes;
    return a > b ? a : b;
}

size_t ofx_raft_workspace_bytes_mode(const ofx_raft* r, int n_images, int B, int H, int W, int flags) {
    if (n_images < 0 || B <= 0 || H <= 0 || W <= 0 || (H % 8) || (W % 8) || flags < 0 || flags >= 2 * OFX_RAFT_F16) return 0;
    if (n_images > 0 && (flags & (OFX_RAFT_SHARED_IMG1 | OFX_RAFT_SHARED_IMG2))) return 0;
    const int layout = flags & (OFX_RAFT_ALT_CORR | OFX_RAFT_SHARED_IMG1 | OFX_RAFT_SHARED_IMG2);
    if (r && r->variant == 1) return small_workspace_bytes_mode(B, H, W, layout, n_images);
    return carve(nullptr, 0, B, H, W, layout, n_images).bytes;
}

size_t ofx_raft_workspace_bytes_pairs(const ofx_raft* r, int n_images, int B, int H, int W) {
    if (n_images <= 0 || B <= 0 || H <= 0 || W <= 0 || (H % 8) || (W % 8)) return 0;
    if (r && r->variant == 1) return small_workspace_bytes(B, H, W, n_images);
    return carve(nullptr, 0, B, H, W, 0, n_images).bytes;
}

// the one way into the four forwards: the argument checks, then the network's plain or indexed-pairs body
static int forward_call(ofx_raft* r, Call c, bool pairs) {
    OFX_REQUIRE(r, OFX_EINVAL);
    const bool small = r->variant == 1;
    const int st = parse_call(&c, pairs, small ? S_UNSUPPORTED : 0);
    if (st) return st;
    if (pairs) return small ? small_forward_pairs(r, c) : basic_forward_pairs(r, c);
    return small ? small_forward(r, c) : basic_forward(r, c);
}

int ofx_raft_forward(ofx_raft* r, const uint8_t* image1, const uint8_t* image2, int B, int H, int W, int iters,
                     int flags, float* flow_up, float* flow_low, void* workspace, size_t workspace_bytes, void* stream) {
    return forward_call(r, {.image1 = image1, .image2 = image2, .B = B, .H = H, .W = W, .iters = iters, .flags = flags, .flow_up = flow_up,
                            .flow_low = flow_low, .workspace = workspace, .workspace_bytes = workspace_bytes, .s = (hipStream_t)stream}, false);
}

int ofx_raft_forward_warp(ofx_raft* r, const uint8_t* image1, const uint8_t* image2, int B, int H, int W, int iters, int flags,
                          float* flow_up, float* flow_low, const uint8_t* warp_frame, float warp_sign, uint8_t* warped, void* workspace,
                          size_t workspace_bytes, void* stream) {
    // every pair is warped: n_warp = B
    return forward_call(r, {.image1 = image1, .image2 = image2, .B = B, .H = H, .W = W, .iters = iters, .flags = flags, .flow_up = flow_up,
                            .flow_low = flow_low, .warp_frame = warp_frame, .warp_sign = warp_sign, .n_warp = B, .warped = warped,
                            .workspace = workspace, .workspace_bytes = workspace_bytes, .s = (hipStream_t)stream}, false);
}

int ofx_raft_forward_pairs(ofx_raft* r, const uint8_t* images, int n_images, const int* idx1, const int* idx2, int B, int H,
                           int W, int iters, int flags, float* flow_up, float* flow_low, void* workspace,
                           size_t workspace_bytes, void* stream) {
    return ofx_raft_forward_pairs_warp(r, images, n_images, idx1, idx2, B, H, W, iters, flags, flow_up, flow_low, nullptr, 1.0f, 0, nullptr,
                                       workspace, workspace_bytes, stream);
}

int ofx_raft_forward_pairs_warp(ofx_raft* r, const uint8_t* images, int n_images, const int* idx1, const int* idx2, int B, int H,
                                int W, int iters, int flags, float* flow_up, float* flow_low, const uint8_t* warp_frame, float warp_sign,
                                int n_warp, uint8_t* warped, void* workspace, size_t workspace_bytes, void* stream) {
    return forward_call(r, {.image1 = images, .n_images = n_images, .idx1 = idx1, .idx2 = idx2, .B = B, .H = H, .W = W, .iters = iters,
                            .flags = flags, .flow_up = flow_up, .flow_low = flow_low, .warp_frame = warp_frame, .warp_sign = warp_sign,
                            .n_warp = n_warp, .warped = warped, .workspace = workspace, .workspace_bytes = workspace_bytes,
                            .s = (hipStream_t)stream}, true);
}

int ofx_raft_variant(const ofx_raft* r) {
    OFX_REQUIRE(r, OFX_EINVAL);
    return r->variant;
}

int ofx_raft_buffer(const ofx_raft* r, const char* name, void** ptr, size_t* nfloats) {
    OFX_REQUIRE(r && name && ptr && nfloats, OFX_EINVAL);
    auto it = r->bufs.find(name);
    if (it == r->bufs.end()) return OFX_EKEY;
    *ptr = it->second.first;
    *nfloats = it->second.second;
    return 0;
}

}  // extern "C"
