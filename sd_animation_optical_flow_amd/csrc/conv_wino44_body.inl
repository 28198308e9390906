// The body of the F(4x4,3x3) kernels (conv_wino.hip, where the design is described): included into wino44_conv_kernel with NORM =
// RES = STATS = false and into the template wino44_fused_kernel<NORM, RES, STATS>.  The enclosing kernel provides `p` (WinoK),
// `smem44` (kSmem44 bytes of dynamic LDS) and the three constants.  Shared as text, not as a __device__ function: inlined from a
// function the plain kernel compiles to another register allocation and schedule, and its assembly is held fixed
// (tests/test_wino44_isa_schedule.py, tools/wino44_bits.py).
    using HALO = Halo44;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: the weight offsets and the row coefficients stay scalar
    const int wi = wave >> 1, nt = wave & 1;
    const Patch pt = wino_patch<16, 32>(p);

    // ---- halo staging: item i = tid + 768 k = (pixel i / 2, float4 slot i % 2), pixels row-major over the halo
    const float* in1s = p.in1 ? p.in1 : p.in0;
    const int bytes1s = p.in1 ? p.bytes1 : p.bytes0;
    // A thread keeps, for each of its two items, the pixel's index in the map (-1: out of the map, or no item) and its place in
    // the halo image: with the row transform staged, the 168 registers of three waves per SIMD hold them next to 96 accumulators.
    // Item 1 is 384 pixels = 11 rows and 10 pixels on.
    static_assert(HALO::slots == 2 && HALO::threads / 2 == 11 * HALO::W + 10, "item 1 = item 0 + 11 rows + 10 pixels");
    int hpix[HALO::slots], hat[HALO::slots];
#pragma unroll
    for (int k = 0; k < HALO::slots; ++k) {
        const int px = (tid >> 1) + k * (HALO::threads / 2);
        const int hy = px / HALO::W, hx = px - hy * HALO::W;
        const int gy = pt.y0 - 1 + hy, gx = pt.x0 - 1 + hx;
        const bool item = k == 0 || tid < HALO::items - HALO::threads;
        hpix[k] = item && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W ? (pt.pb * p.H + gy) * p.W + gx : -1;
        hat[k] = item ? HALO::at(hy, hx) + (tid & 1) * 4 : -1;   // (float4 slot tid % 2 of the pixel: 768 % 2 == 0, the same for both)
    }
    auto h_issue = [&](int cb, float4 (&r)[HALO::slots]) __attribute__((always_inline)) {
        const int c = cb * 8;
        const bool s0 = c < p.c0;    // wave-uniform
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(s0 ? p.in0 : in1s), (short)0, s0 ? p.bytes0 : bytes1s, 0x00020000);
        const int so = (s0 ? c : c - p.c0) * 4;
        const int ldb = (s0 ? p.ld0 : p.ld1) * 4;
#pragma unroll
        for (int k = 0; k < HALO::slots; ++k) {
            const int vo = hpix[k] >= 0 ? hpix[k] * ldb + (tid & 1) * 16 : kOOB;
            v4i t = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, so, 0);
            r[k] = *reinterpret_cast<float4*>(&t);
        }
    };
    // (cb: the slab in r; NORM reads its thread's four means and rstds of it from Ns, and the padding stays zero)
    const float* const Ns = smem44 + kStage44 + (tid & 1) * 8;
    auto h_store = [&](float* Hs, const float4 (&r)[HALO::slots], int cb) __attribute__((always_inline)) {
        float4 mu, rs;
        if constexpr (NORM) {
            mu = *reinterpret_cast<const float4*>(Ns + cb * 16);
            rs = *reinterpret_cast<const float4*>(Ns + cb * 16 + 4);
        }
#pragma unroll
        for (int k = 0; k < HALO::slots; ++k)
            if (k == 0 || hat[k] >= 0) {   // (quads 34 floats apart: 8-byte aligned)
                float* const at = Hs + hat[k];
                float4 v = r[k];
                if constexpr (NORM) {   // as HaloStage::store
                    v.x = fmaxf((v.x - mu.x) * rs.x, 0.f);
                    v.y = fmaxf((v.y - mu.y) * rs.y, 0.f);
                    v.z = fmaxf((v.z - mu.z) * rs.z, 0.f);
                    v.w = fmaxf((v.w - mu.w) * rs.w, 0.f);
                    if (hpix[k] < 0) v = make_float4(0.f, 0.f, 0.f, 0.f);
                }
                *reinterpret_cast<float2*>(at) = f2(v.x, v.y);
                *reinterpret_cast<float2*>(at + 2) = f2(v.z, v.w);
            }
    };

    // ---- the row pass: row i of B^T d, i = 0 .. 5, for the windows of tile row ty, once per workgroup.  Thread `tid` < 544 owns
    // (ty, x, channel pair): the window's six halo rows 4 ty .. 4 ty + 5 at pixel x, six results.  Rows 1 .. 4 take halo rows
    // 1 .. 4, t = c0 d1 + c1 d2 + c2 d3 + c3 d4; rows 0 and 5 take rows (0, 2, 4) and (1, 3, 5), t = 4 d0 - 5 d1 + d2.  The
    // expressions keep the form and the operand order they had when every wave worked its own row out: the same bits.
    const int rpx = tid >> 2, rty = rpx / HALO::W, rx = rpx - rty * HALO::W;
    const int rxo = (rx >> 2) * HALO::lquad + (rx & 3) * 8 + (tid & 3) * 2;
    const int rin = tid < HALO::titems ? 4 * rty * HALO::lrow + rxo : -1, rout = rty * HALO::ltrow + rxo;
    auto row_pass = [&](const float* Rs, float* Ts, bool on) __attribute__((always_inline)) {
        if (rin >= 0 && on) {
            const float* const d = Rs + rin;
            float* const o = Ts + rout;
            float2 r[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) r[k] = *reinterpret_cast<const float2*>(d + k * HALO::lrow);
            __builtin_amdgcn_sched_barrier(0);   // all six reads in flight before the first result is stored
            auto outer = [](float d0, float d1, float d2) { return __builtin_fmaf(-5.f, d1, __builtin_fmaf(4.f, d0, d2)); };
            auto inner = [](float c0, float c1, float c2, float c3, float d0, float d1, float d2, float d3) {
                return __builtin_fmaf(c3, d3, __builtin_fmaf(c2, d2, __builtin_fmaf(c1, d1, c0 * d0)));
            };
#define OFX_ROW44(i, EX, EY) *reinterpret_cast<float2*>(o + (i) * 4 * HALO::ltrow) = f2(EX, EY)
            OFX_ROW44(0, outer(r[0].x, r[2].x, r[4].x), outer(r[0].y, r[2].y, r[4].y));
            OFX_ROW44(1, inner(-4.f, -4.f, 1.f, 1.f, r[1].x, r[2].x, r[3].x, r[4].x), inner(-4.f, -4.f, 1.f, 1.f, r[1].y, r[2].y, r[3].y, r[4].y));
            OFX_ROW44(2, inner(4.f, -4.f, -1.f, 1.f, r[1].x, r[2].x, r[3].x, r[4].x), inner(4.f, -4.f, -1.f, 1.f, r[1].y, r[2].y, r[3].y, r[4].y));
            OFX_ROW44(3, inner(-2.f, -1.f, 2.f, 1.f, r[1].x, r[2].x, r[3].x, r[4].x), inner(-2.f, -1.f, 2.f, 1.f, r[1].y, r[2].y, r[3].y, r[4].y));
            OFX_ROW44(4, inner(2.f, -1.f, -2.f, 1.f, r[1].x, r[2].x, r[3].x, r[4].x), inner(2.f, -1.f, -2.f, 1.f, r[1].y, r[2].y, r[3].y, r[4].y));
            OFX_ROW44(5, outer(r[1].x, r[3].x, r[5].x), outer(r[1].y, r[3].y, r[5].y));
#undef OFX_ROW44
        }
    };
    // the product side: wave (i, nt) reads row i of T only, one float2 per window column and half-step
    const int tile = lane & 31;
    const int at0 = (wi * 4 + (tile >> 3)) * HALO::ltrow + (tile & 7) * HALO::lquad + 4 * (lane >> 5);
    auto t_read = [&](const float* Tw, int s, float2 (&t)[6]) __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < 6; ++c) t[c] = *reinterpret_cast<const float2*>(Tw + HALO::at(0, c) + 2 * s);
    };

    // the weights: point 6 i + j, 32-channel block blk, 8-channel chunk cb, half s -> one contiguous 512-byte fragment, 8 bytes per
    // lane (ofx_wino44_conv_weight); step (cb, s) = 2 cb + s
    const __amdgpu_buffer_rsrc_t rsu = __builtin_amdgcn_make_buffer_rsrc((void*)p.u, (short)0, p.bytesu, 0x00020000);
    const int c8n = p.cin >> 3;
    const int fr0 = (6 * wi * p.nb32 + 2 * pt.nb + nt) * c8n * 2, frq = p.nb32 * c8n * 2;   // fragments: point row's first, per point
    auto w_load = [&](int j, int step) __attribute__((always_inline)) {
        typedef int v2i __attribute__((ext_vector_type(2)));
        v2i t = __builtin_amdgcn_raw_buffer_load_b64(rsu, lane * 8, (fr0 + j * frq + step) * 512, 0);
        return *reinterpret_cast<float2*>(&t);
    };
    f32x16 acc[6][1];
    wino_zero(acc);
    float2 wr[6];

    // LDS: raw halo slabs R[2], then T[2].  Trip k, after its barrier: raw slab k + 2 goes from registers into R[k % 2] (last read
    // by the row pass of trip k - 1), the loads of slab k + 3 are issued, the row pass takes raw slab k + 1 (stored in trip k - 1)
    // from R[(k + 1) % 2] into T[(k + 1) % 2] (last read by the products of trip k - 1), and the products of slab k read
    // T[k % 2]: one barrier per slab.
    float* const Hs = smem44;
    float* const Ts = smem44 + 2 * HALO::floats;
    const int CB = p.cin >> 3;
    float4 h0[HALO::slots], hn[HALO::slots];
    h_issue(0, h0);
    h_issue(1, hn);
    if constexpr (NORM) {   // the image's means and rstds, under the first halo loads
        float* const ns = smem44 + kStage44;
        for (int c = tid; c < p.cin; c += HALO::threads) {
            ns[(c >> 2) * 8 + (c & 3)] = p.nmean[(long)pt.pb * p.c0 + c];
            ns[(c >> 2) * 8 + 4 + (c & 3)] = p.nrstd[(long)pt.pb * p.c0 + c];
        }
        __syncthreads();
    }
    h_store(Hs, h0, 0);
    h_store(Hs + HALO::floats, hn, 1);
    h_issue(CB > 2 ? 2 : CB - 1, hn);
    // (the weights after the last halo loads, as in the loop: the first trip's halo wait then leaves them in flight too)
#pragma unroll
    for (int j = 0; j < 6; ++j) wr[j] = w_load(j, 0);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    row_pass(Hs, Ts, true);
    const float* const T0 = Ts + at0;
    // the six column points of a row: the same combinations along the window's columns, one channel at a time
    auto fold = [&](const float2 (&t)[6], float (&v)[2][6]) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            float x[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) x[c] = e ? t[c].y : t[c].x;
            const float A = __builtin_fmaf(-4.f, x[2], x[4]), Bq = __builtin_fmaf(-4.f, x[1], x[3]), C = x[4] - x[2], D = x[3] - x[1];
            v[e][0] = __builtin_fmaf(4.f, x[0], __builtin_fmaf(-5.f, x[2], x[4]));
            v[e][1] = A + Bq;
            v[e][2] = A - Bq;
            v[e][3] = __builtin_fmaf(2.f, D, C);
            v[e][4] = __builtin_fmaf(-2.f, D, C);
            v[e][5] = __builtin_fmaf(4.f, x[1], __builtin_fmaf(-5.f, x[3], x[5]));
        }
    };
    // two slabs per trip (whole 16-channel slabs: CB is even), so that the buffer of each is a constant offset
#pragma clang loop unroll(disable)
    for (int cb2 = 0; cb2 < CB; cb2 += 2)
#pragma unroll
    for (int par = 0; par < 2; ++par) {
        const int cb = cb2 + par;
        __syncthreads();   // slab cb's T is in buffer par, raw slab cb + 1 in the other raw buffer, and every wave has left the rest
        float2 t[2][6];
        t_read(T0 + par * HALO::tfloats, 0, t[0]);
        if constexpr (NORM) h_store(Hs + par * HALO::floats, hn, cb + 2 < CB ? cb + 2 : CB - 1);
        else h_store(Hs + par * HALO::floats, hn, 0);
        // the last slabs re-issue the last one (and store it where nothing reads it): no branch, loads stay in bounds
        h_issue(cb + 3 < CB ? cb + 3 : CB - 1, hn);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float v[2][6];
            if (s == 1) __builtin_amdgcn_sched_barrier(0);   // (its operands are waited for behind the first half's MFMAs)
            fold(t[s], v);
            if (s == 0) {
                // the second half-step's six reads go under the first one's MFMAs
                __builtin_amdgcn_sched_barrier(0);
                t_read(T0 + par * HALO::tfloats, 1, t[1]);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (s == 1) {
                // The row pass of the next slab (not of the one past the last) sits between the two half-steps: its wave has twelve
                // MFMAs queued and the SIMD's other waves have the matrix pipe.  The second half's operands are folded first
                // (the empty asm keeps the fold on this side of the branch), so that no MFMA waits for the LDS stores behind it.
#pragma unroll
                for (int e = 0; e < 2; ++e)
#pragma unroll
                    for (int j = 0; j < 6; ++j) asm volatile("" : "+v"(v[e][j]));
                row_pass(Hs + (1 - par) * HALO::floats, Ts + (1 - par) * HALO::tfloats, cb + 1 < CB);
                __builtin_amdgcn_sched_barrier(0);
            }
            const int nx = 2 * cb + s + 1 < 2 * CB ? 2 * cb + s + 1 : 2 * cb + s;
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    acc[j][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[e][j], e ? wr[j].y : wr[j].x, acc[j][0], 0, 0, 0);
                    if (e) {
                        // the next step's fragment goes into the registers these MFMAs have just read, ten MFMAs ahead of its use,
                        // and stays there (as in wino3x3_slabs: left free, the scheduler sinks the loads to their uses)
                        wr[j] = w_load(j, nx);
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                    }
                }
        }
    }

    // ---- output transform and epilogue.  A^T (4x6) along the column in registers, the six rows meet in LDS, half of the
    // patch's tiles (two tile rows) at a time: X[wave][b][tile][channel].  Element e of the C layout: tile (e & 3) + 8 (e >> 2) +
    // 4 (lane >> 5), output channel lane & 31 of the wave's 32.
    //
    // The row side: a lane takes four adjacent output channels of one pixel, rows ap and ap + 2 of its tile -- five ds_read_b128
    // (point rows ap .. ap + 4) and two 16-byte stores; eight lanes cover a pixel's 32 channels, one 128-byte line.  A wave's unit
    // is (channel half ont, row pair ap, tiles tl = {t, t + 4} of one tile row, columns b = 0 .. 3): 32 units per half of the
    // patch, unit wave + 12 k in pass k, so that ont = wave & 1 and ap = (wave >> 1) & 1 hold for all of a wave's units and are
    // scalar: one transform per wave behind a scalar branch, scale / shift read once.  Lane = (channel quad lane & 7, b & 1 at bit
    // 3, tl & 4 at bit 4, b >> 1 at bit 5): with X as the accumulator side writes it (conflict-free: 32 consecutive floats per
    // half-wave), a 16-lane group of the ds_read_b128 takes the low half of one row and the high half of the row 16 on (640
    // floats: the same banks), and the high and low halves of the two rows four on (160 floats: 32 banks on) -- 16 different bank
    // quads (tools/lds_bank_model.py --wino44-exchange).
    // Addresses: a scalar 64-bit base per pass (image, patch, tile row and column, channel block) and one 32-bit byte offset per
    // lane that never changes, (16 (tl & 4) / 4 + b) pixels and the channel quad: at most 32 ldo floats.  A quad is stored as
    // 16 bytes where the host found the destination (and scale, shift, res) aligned for it (p.vec4) and the quad whole; a quad
    // that straddles Cout, and every quad of an unaligned destination, goes channel by channel and writes nothing from Cout on.
    // Every output is computed by the operations, in the order, of the one-channel-per-lane form this replaces: the same bits.
    const float act_lo = p.act == OFX_ACT_RELU ? 0.0f : -3.402823466e38f;   // OFX_ACT_NONE: a NaN sum becomes -FLT_MAX (see conv.hip)
    float* const X = smem44;
    const int ont = wave & 1, ap = (wave >> 1) & 1;
    const int cq = lane & 7, ob = ((lane >> 3) & 1) + 2 * (lane >> 5), t2 = (lane >> 4) & 1;
    const int oc0 = pt.nb * 64 + ont * 32 + 4 * cq;
    const int nv = p.Cout - oc0;            // how many of the quad's channels exist (<= 0: none)
    const bool quad = p.vec4 && nv >= 4;
    float sc[4], sh[4];                     // under the column side below
    if (quad) {
        const float4 s4 = p.scale ? *reinterpret_cast<const float4*>(p.scale + oc0) : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        const float4 h4 = p.shift ? *reinterpret_cast<const float4*>(p.shift + oc0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        sc[0] = s4.x, sc[1] = s4.y, sc[2] = s4.z, sc[3] = s4.w;
        sh[0] = h4.x, sh[1] = h4.y, sh[2] = h4.z, sh[3] = h4.w;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            sc[c] = p.scale && c < nv ? p.scale[oc0 + c] : 1.0f;
            sh[c] = p.shift && c < nv ? p.shift[oc0 + c] : 0.0f;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) sc[c] *= p.alpha;
    const int xlane = (ob * 16 + t2 * 4) * kLDX4 + 4 * cq;
    const unsigned olane = (unsigned)((16 * t2 + ob) * p.ldo + ont * 32 + 4 * cq) * 4u;   // bytes
    char* const out0 = reinterpret_cast<char*>(p.out + (((long)pt.pb * p.H + pt.y0) * p.W + pt.x0) * p.ldo + pt.nb * 64);
    const long orow_b = (long)p.W * p.ldo * 4;   // a pixel row of the destination, bytes
    unsigned rlane = 0;
    const char* res0 = nullptr;
    long rrow_b = 0;
    if constexpr (RES) {
        rlane = (unsigned)((16 * t2 + ob) * p.ldres + ont * 32 + 4 * cq) * 4u;
        res0 = reinterpret_cast<const char*>(p.res + (((long)pt.pb * p.H + pt.y0) * p.W + pt.x0) * p.ldres + pt.nb * 64);
        rrow_b = (long)p.W * p.ldres * 4;
    }
    typedef float v2f __attribute__((ext_vector_type(2)));
    struct Ap0 { enum { v = 0 }; };
    struct Ap1 { enum { v = 1 }; };
    // STATS: the lane's four channels, every value it stores, in the order of its units
    float st_s[4] = {0.0f, 0.0f, 0.0f, 0.0f}, st_q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        __syncthreads();   // half 0: every wave's last operand reads are done; half 1: the first half has been read
#pragma unroll
        for (int eh = 0; eh < 8; ++eh) {
            const int e = 8 * half + eh;
            const int tl = (e & 3) + 8 * ((e >> 2) & 1) + 4 * (lane >> 5);
            const float m0 = acc[0][0][e], m1 = acc[1][0][e], m2 = acc[2][0][e], m3 = acc[3][0][e], m4 = acc[4][0][e], m5 = acc[5][0][e];
            const float s12 = m1 + m2, d12 = m1 - m2, s34 = m3 + m4, d34 = m3 - m4;
            float* const x = X + (wave * 4 * 16 + tl) * kLDX4 + (lane & 31);
            x[0 * 16 * kLDX4] = m0 + s12 + s34;
            x[1 * 16 * kLDX4] = d12 + 2.0f * d34;
            x[2 * 16 * kLDX4] = s12 + 4.0f * s34;
            x[3 * 16 * kLDX4] = d12 + 8.0f * d34 + m5;
        }
        __syncthreads();
        // pass k: unit wave + 12 k = (ont, ap, ts = wave / 4 + 3 k: tile column ts & 3 (and + 4), tile row ts >> 2 of the half);
        // waves 8 .. 11 have two.  One copy of the pass per row pair: AP is a constant in it.
        auto row_side = [&](auto apc) __attribute__((always_inline)) {
            constexpr int AP = decltype(apc)::v;
#pragma clang loop unroll(disable)
            for (int ts = wave >> 2; ts < 8; ts += 3) {
                const int orow = 4 * (2 * half + (ts >> 2)) + AP, ocol = 4 * (ts & 3);   // the unit's first pixel in the patch
                char* const oa = out0 + orow * orow_b + (long)(ocol * p.ldo) * 4;
                char* const ob2 = oa + 2 * orow_b;
                float ra[4] = {0.0f, 0.0f, 0.0f, 0.0f}, rb[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // RES: in flight under the exchange reads
                if constexpr (RES) {
                    const char* const qa = res0 + orow * rrow_b + (long)(ocol * p.ldres) * 4;
                    const char* const qb = qa + 2 * rrow_b;
                    if (quad) {
                        const float4 a4 = *reinterpret_cast<const float4*>(qa + rlane), b4 = *reinterpret_cast<const float4*>(qb + rlane);
                        ra[0] = a4.x, ra[1] = a4.y, ra[2] = a4.z, ra[3] = a4.w;
                        rb[0] = b4.x, rb[1] = b4.y, rb[2] = b4.z, rb[3] = b4.w;
                    } else {
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            if (c < nv) {
                                ra[c] = reinterpret_cast<const float*>(qa + rlane)[c];
                                rb[c] = reinterpret_cast<const float*>(qb + rlane)[c];
                            }
                    }
                }
                // rows AP .. AP + 4 of the point grid, the quad's channels as two pairs (packed fp32: the same roundings)
                v2f x[2][5];
                const float* const xu = X + ((AP * 2 + ont) * 4 * 16 + (ts & 3) + 8 * (ts >> 2)) * kLDX4 + xlane;
#pragma unroll
                for (int r = 0; r < 5; ++r) {
                    const float4 t = *reinterpret_cast<const float4*>(xu + r * (2 * 4 * 16 * kLDX4));
                    x[0][r] = v2f{t.x, t.y};
                    x[1][r] = v2f{t.z, t.w};
                }
                float va[4], vb[4];   // output rows AP and AP + 2
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const v2f(&xp)[5] = x[h];
                    v2f ya, yb;
                    if constexpr (AP == 0) {
                        ya = xp[0] + (xp[1] + xp[2]) + (xp[3] + xp[4]);
                        yb = (xp[1] + xp[2]) + 4.0f * (xp[3] + xp[4]);
                    } else {
                        ya = (xp[0] - xp[1]) + 2.0f * (xp[2] - xp[3]);
                        yb = (xp[0] - xp[1]) + 8.0f * (xp[2] - xp[3]) + xp[4];
                    }
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int c = 2 * h + e;
                        va[c] = fmaxf(__builtin_fmaf(ya[e], sc[c], sh[c]), act_lo);
                        vb[c] = fmaxf(__builtin_fmaf(yb[e], sc[c], sh[c]), act_lo);
                        if constexpr (RES) {
                            va[c] = fmaxf(va[c] + ra[c], 0.0f);
                            vb[c] = fmaxf(vb[c] + rb[c], 0.0f);
                        }
                        if constexpr (STATS) {
                            st_s[c] += va[c];
                            st_q[c] = fmaf(va[c], va[c], st_q[c]);
                            st_s[c] += vb[c];
                            st_q[c] = fmaf(vb[c], vb[c], st_q[c]);
                        }
                    }
                }
                if (quad) {
                    *reinterpret_cast<float4*>(oa + olane) = make_float4(va[0], va[1], va[2], va[3]);
                    *reinterpret_cast<float4*>(ob2 + olane) = make_float4(vb[0], vb[1], vb[2], vb[3]);
                } else if (nv > 0) {   // (nested, not a run of ifs: forward branches only)
                    float* const pa = reinterpret_cast<float*>(oa + olane);
                    float* const pb = reinterpret_cast<float*>(ob2 + olane);
                    pa[0] = va[0], pb[0] = vb[0];
                    if (nv > 1) {
                        pa[1] = va[1], pb[1] = vb[1];
                        if (nv > 2) {
                            pa[2] = va[2], pb[2] = vb[2];
                            if (nv > 3) pa[3] = va[3], pb[3] = vb[3];
                        }
                    }
                }
            }
        };
        if (ap == 0) row_side(Ap0{});
        else row_side(Ap1{});
    }
    if constexpr (STATS) {   // a channel's 48 partials (six waves, eight lanes each) meet in LDS and are added in index order
        __syncthreads();     // the last exchange has been read
        float* const Sx = smem44;
        float* const sx = Sx + (((ont * 48 + (wave >> 1) * 8 + (lane >> 3)) * 32) + 4 * cq) * 2;
        *reinterpret_cast<float4*>(sx) = make_float4(st_s[0], st_q[0], st_s[1], st_q[1]);
        *reinterpret_cast<float4*>(sx + 4) = make_float4(st_s[2], st_q[2], st_s[3], st_q[3]);
        __syncthreads();
        const int grp = tid >> 5, on = tid & 31;
        const int oc = pt.nb * 64 + grp * 32 + on;
        if (tid < 64 && oc < p.Cout) {
            float s = 0.0f, q = 0.0f;
            for (int g = 0; g < 48; ++g) {
                s += Sx[((grp * 48 + g) * 32 + on) * 2 + 0];
                q += Sx[((grp * 48 + g) * 32 + on) * 2 + 1];
            }
            const long row = (long)pt.pb * p.tpi + (pt.y0 >> 4) * p.tpr + (pt.x0 >> 5);
            p.stats[(row * p.Cout + oc) * 2 + 0] = s;
            p.stats[(row * p.Cout + oc) * 2 + 1] = q;
        }
    }
