/*
 * ofx.h -- C ABI of the MI355X-native optical-flow hot path (libofx.so).
 *
 * Drop-in boundary for the flow / warp / mask path of zyddnys/sd_animation_optical_flow.
 * Every entry point takes plain device pointers and sizes plus a `hipStream_t` passed as void*;
 * there are no torch types in any signature.  All functions return 0 on success, a positive
 * hipError_t on a HIP failure, or a negative OFX_E* code on a precondition failure (the reference's
 * TORCH_CHECKs, RAFT/alt_cuda_corr/correlation.cpp:19-21, become return codes).  Work is enqueued
 * on the given stream and is asynchronous, like the reference's launches.
 *
 * Reference interface each group replaces (file:line relative to the reference repo):
 *   ofx_local_corr_fwd          RAFT/alt_cuda_corr/correlation.cpp:23-33,51-54  (alt_cuda_corr.forward)
 *                               RAFT/alt_cuda_corr/correlation_kernel.cu:18-119,260-286
 *   ofx_corr_volume / _lookup   RAFT/core/corr.py:13-60   (CorrBlock)
 *   ofx_conv2d, ofx_inorm_*     RAFT/core/extractor.py:118-192, RAFT/core/update.py:6-136
 *   ofx_upsample_flow           RAFT/core/raft.py:72-83
 *   ofx_raft_*                  RAFT/core/raft.py:86-144 ; ofgen_keyframe_inpaint.py:47-71 (RAFT_2)
 *   ofx_warp_*                  pdcnet_of.py:34-42 ; ofgen_keyframe_inpaint.py:92-98 (cv2.remap)
 *   ofx_generate_mask, ofx_dilate_u8, ofx_expand_mask, ofx_travel_distance, ofx_flow_magnitude, ofx_merge_images,
 *   ofx_mix_frames, ofx_conf_sum
 *   ofx_groupnorm, ofx_softmax_rows, ofx_attention_f32, ofx_attention_prec
 *   ofx_upconv2x, ofx_upconv2x_prec, ofx_upsample2x_nearest_f32, ofx_decode_to_u8
 *                               ldm/modules/diffusionmodules/model.py:35-41,152-203 ; ldm/modules/attention.py:314,426
 *   ofx_layernorm, ofx_geglu, ofx_attention_bnhd_f32, ofx_attention_bnhd_prec
 *                               ldm/modules/attention.py:54-56,326-436,456-469,515-537 (SpatialTransformer)
 *                               ofgen_keyframe_inpaint.py:113-133,237-248,306-322,676-688,968-973,995-1027
 *   ofx_groupnorm_cat, ofx_emb_linear, ofx_timestep_embedding
 *                               ldm/modules/diffusionmodules/openaimodel.py:220-226,257-277,530-534,757-793 ; util.py:154-174
 *   ofx_ddim_step               guided_ldm_inpainting.py:28-137,337-338 ; guided_ldm.py:82-89,123
 *   ofx_conv3x3_silu            controlnet.py:164-180 (ControlNet.input_hint_block)
 *   ofx_clip_embed, ofx_quick_gelu
 *                               hack.py:32-70 (_hacked_clip_forward) ; ldm/modules/encoders/modules.py (FrozenCLIPEmbedder)
 *
 * Layout conventions: images and flow are HWC ("channels-last"); network activations are
 * NHWC fp32; a flow field is f32[H,W,2] = (dx, dy) exactly as `algo.calc` returns it
 * (pdcnet_of.py:72).
 */
#ifndef OFX_H
#define OFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFX_VERSION 100

/* negative error codes (positive values are hipError_t) */
#define OFX_EINVAL   (-1)   /* bad argument (null pointer, non-positive size, unsupported mode) */
#define OFX_EALIGN   (-2)   /* pointer / leading dimension not 16-byte aligned where required   */
#define OFX_ENOMEM   (-3)   /* workspace too small                                             */
#define OFX_EKEY     (-4)   /* weight tensor missing or of the wrong shape                      */
#define OFX_ENODEV   (-5)   /* no gfx950 device                                                 */

int ofx_version(void);
const char* ofx_error_string(int code);

/* ---------------------------------------------------------------- profiling (HIP events) */
/* When enabled, every kernel launch issued through this library is bracketed by a pair of
 * hipEvents recorded on the launch stream.  ofx_prof_collect synchronises, accumulates the elapsed
 * times per kernel name and writes a JSON object {"name": {"calls": n, "ms": total, "flops": executed}, ...}
 * ("flops" is non-zero for the GEMM/conv launches).
 * on = 1: one entry per kernel family; on = 2: the RAFT executor's convolutions are split per layer
 * ("family:layer"). */
int ofx_prof_enable(int on);
int ofx_prof_collect(char* json_out, size_t cap);

/* ---------------------------------------------------------------- warp */
#define OFX_WARP_BILINEAR  0   /* grid_sample(bilinear, zeros, align_corners=True) semantics  */
#define OFX_WARP_BICUBIC   1   /* float Keys cubic A=-0.75, zero border                        */
#define OFX_WARP_CV2_CUBIC 2   /* OpenCV remap INTER_CUBIC: 1/32-px coords, 15-bit weights     */

/* out[b,y,x,:] = frame[b', y + sign*flow[b,y,x,1], x + sign*flow[b,y,x,0], :].
 * frame_bstride = elements between consecutive frames (0 = one shared key frame for all B flows).
 * sign = +1: pdcnet_of.warp_frame; sign = -1: the RAFT-convention warp_frame. C in [1,4]. */
int ofx_warp_u8(const uint8_t* frame, long frame_bstride, const float* flow, uint8_t* out,
                int B, int H, int W, int C, int mode, float sign, void* stream);
int ofx_warp_f32(const float* frame, long frame_bstride, const float* flow, float* out,
                 int B, int H, int W, int C, int mode, float sign, void* stream);
/* cv2.resize(INTER_CUBIC) of an f32 HWC image (used by warp_frame_latent, pdcnet_of.py:24,30) */
int ofx_resize_cubic_f32(const float* src, float* dst, int B, int Hs, int Ws, int Hd, int Wd, int C,
                         void* stream);

/* ---------------------------------------------------------------- masks */
/* mask = dilate(255*(conf < thres), ellipse ksize); if log_conf != NULL, log_conf[conf<thres] = 0
 * in place (generate_mask, ofgen_keyframe_inpaint.py:317-322).  cmp_gt = 0: low = conf < thres;
 * cmp_gt = 1: low = !(conf > thres) (the keyframe path's convention, :995). ksize odd, <= 31;
 * ksize = 1 means no dilation. */
int ofx_generate_mask(const float* conf, float* log_conf, uint8_t* mask, int B, int H, int W,
                      float thres, int ksize, int cmp_gt, void* stream);
int ofx_dilate_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, int ksize, void* stream);
/* out = mask | dilate(255*(gray(|laplacian(image)| mod 256) > edge_thres), ellipse ksize) */
int ofx_expand_mask(const uint8_t* mask, const uint8_t* image_bgr, uint8_t* out, uint8_t* scratch,
                    int B, int H, int W, int edge_thres, int ksize, void* stream);
/* The kernel and launch shape ofx_generate_mask / ofx_warp_and_mask (src 0: conf < thres, 1: !(conf > thres)) or ofx_expand_mask
 * (src 3: Laplacian edges) take for B images of H x W and an odd ksize <= 31, without launching: the launcher calls this and
 * launches what it says.  aligned16: whether every pointer of the call (confidence, output and, when given, the mask ORed in) is
 * 16-byte aligned.  Only numbers are looked at: no device is needed.  Succeeds for every shape the entry points accept with
 * B <= 65535 (the tile kernels put the image index on the grid's z axis); OFX_EINVAL otherwise. */
#define OFX_MASK_KERNEL_ROWS   0   /* full-width bands of one image: confidence sources, W % 4 == 0, W <= 4096, aligned16 */
#define OFX_MASK_KERNEL_NARROW 1   /* 56 x 32 ballot tiles: ksize <= 9 */
#define OFX_MASK_KERNEL_WIDE   2   /* 64 x 32 ballot tiles */
typedef struct ofx_mask_route {
    int kernel;              /* OFX_MASK_KERNEL_* */
    int band_rows;           /* output rows per workgroup: 64, 32 or 16 (rows kernel), 32 (tile kernels) */
    int threads;             /* per workgroup */
    int nplanes;             /* rows kernel: distinct half-widths > 0 of the element kept as spread planes in LDS (0..8), or -1:
                                direct evaluation (more than 8 of them, or the planes would need more than 48 KiB); tiles: 0 */
    int xcd_map;             /* rows kernel: 1 = workgroup ids laid out so that the bands of an image share an XCD */
    int lds_bytes;           /* dynamic LDS per workgroup (rows kernel; the tile kernels' LDS is static: 0) */
    int workgroups;          /* in the grid, the idle ones of a ragged last XCD group included */
} ofx_mask_route;
int ofx_mask_plan(int src, int B, int H, int W, int ksize, int aligned16, ofx_mask_route* out);
/* v = |flow| with v[conf < conf_floor] = 0 (of_calc, ofgen_keyframe_inpaint.py:118-126) */
int ofx_travel_distance(const float* flow, const float* conf, float* out, int B, int H, int W,
                        float conf_floor, void* stream);
/* The RAFT-variant of_calc (reference ofgen.py:45-49, caller :137): v = sqrt(fx*fx + fy*fy) of a bare flow, n pixels; f32
 * multiply, multiply, add (no contraction) and a correctly rounded square root: numpy's bits. */
int ofx_flow_magnitude(const float* flow, float* out, long n, void* stream);
/* confidence_to_mask (:237-248): travel' = warp(travel, flow) + dist; travel'[conf<0.9] = 0;
 * raw = 255*(conf<0.9 | travel' > thres); travel'[travel'>thres] = 0.  `raw` is un-dilated; the
 * caller dilates with ofx_dilate_u8(ksize=15). travel_in and travel_out must not alias. */
int ofx_travel_mask(const float* conf, const float* flow, const float* dist, const float* travel_in,
                    float* travel_out, uint8_t* raw, int B, int H, int W, float thres, int warp_mode,
                    void* stream);
/* merge_images 'naive' (:676-681): out = base*(1-m) + second*m with m = (mask==255) */
int ofx_merge_images(const uint8_t* base, const uint8_t* second, const uint8_t* mask, uint8_t* out,
                     int B, int H, int W, int C, void* stream);
/* mix_propagated_ai_frame (:306-315): out = raw * (1 - w) + warped * w, w = ppw where mask <= 127, 1 - ppw above; ppw < 0.001:
 * out = raw (:307-308) */
int ofx_mix_frames(const uint8_t* raw, const uint8_t* warped, const uint8_t* mask, uint8_t* out,
                   int B, int H, int W, int C, float ppw, void* stream);
/* sums[n] = sum over HW of conf_like[n, :, :, chan] for a f32[N,H,W,nchan] tensor (f64 accumulate);
 * used for `einops.reduce(flow_mat[...,2], 's t h w -> s', 'sum')` (:666, :1000) */
int ofx_conf_sum(const float* x, double* sums, int N, long HW, int nchan, int chan, void* stream);
/* EXTENSION (no reference counterpart: RAFT emits no confidence and PDCNet+ is not in the reference
 * tree): forward-backward consistency confidence.  flow_fw f32[B,H,W,2] is defined on the target
 * grid, flow_bw on the source grid; e = fw(p) + bw(p + fw(p)); log_conf = -|e|^2/(2 sigma^2);
 * conf = exp(log_conf), shaped like PDCNetPlus.calc's (confidence, log_confidence), pdcnet_of.py:73-74 */
int ofx_fb_confidence(const float* flow_fw, const float* flow_bw, float* conf, float* log_conf, int B,
                      int H, int W, float sigma, void* stream);
/* fused hot-path tail: warped = warp(frame, flow); mask = dilate(255*(conf<thres)) in one call. */
int ofx_warp_and_mask(const uint8_t* frame, long frame_bstride, const float* flow, const float* conf,
                      uint8_t* warped, uint8_t* mask, int B, int H, int W, int C, int warp_mode,
                      float sign, float thres, int ksize, int cmp_gt, void* stream);
/* Greedy multi-reference composition (ofgen_keyframe_inpaint.py:995-1024, the loop shared by the four modes of
 * generate_ai_frame_with_ref) in two launches and without a host read-back.  flow f32[N,H,W,2], conf f32[N,H,W] (raw, not
 * binarised), frames u8[N,H,W,3]; 1 <= N <= 8 and H*W < 2^31 (OFX_EINVAL otherwise).  Pixel p has the pattern
 * b_p = sum_s (conf_s(p) > thres) << s (fp32 compare, NaN = 0).  Round r draws order[r]: the lowest s with the largest number
 * counts[r] of pixels whose bit s is set and none of whose already-drawn bits is set (a drawn reference counts 0; when nothing is
 * left index 0 is drawn again).  select[p] = the first reference in order whose bit is set in b_p, order[0] where b_p == 0 and
 * everywhere with first_only (generate_ai_frame_with_ref_both, :900-908); ret[p] = warp of frames[select[p]] by
 * flow[select[p]] at p, sign +1, the bytes ofx_warp_u8's generic kernel writes; mask[p] = 255 where b_p != 0.
 * ret u8[H,W,3], mask / select u8[H,W], order / counts i32[N].  scratch: ofx_compose_scratch_bytes(N,H,W) bytes, 16-byte
 * aligned (OFX_ENOMEM if smaller; 0 bytes = bad shape). */
size_t ofx_compose_scratch_bytes(int N, int H, int W);
int ofx_compose_refs(const float* flow, const float* conf, const uint8_t* frames, uint8_t* ret, uint8_t* mask,
                     uint8_t* select, int* order, int* counts, void* scratch, size_t scratch_bytes, int N, int H, int W,
                     float thres, int warp_mode, int first_only, void* stream);

/* ---------------------------------------------------------------- SD-inpaint hand-off */
/* What img2img_inpaint derives from (frame, reference, mask) before its first VAE call
 * (ofgen_keyframe_inpaint.py:255-290 -> guided_ldm_inpainting.py:290-316,139-154), bit-exact to Pillow:
 * PIL.ImageFilter.GaussianBlur(radius) on an 8-bit single-channel image [B,H,W] (BoxBlur.c: three extended-box
 * passes per axis).  scratch: B*H*W bytes, distinct from in / out; in == out is allowed. */
int ofx_gaussian_blur_u8(const uint8_t* in, uint8_t* out, uint8_t* scratch, int B, int H, int W, float radius,
                         void* stream);
/* PIL Image.resize((Wout, Hout)) with the default BICUBIC resample on an 8-bit channel (Resample.c: antialiased
 * support, 22-bit fixed-point taps, horizontal pass to 8 bits then vertical).  scratch: B*Hin*Wout bytes. */
int ofx_resize_bicubic_u8(const uint8_t* in, uint8_t* out, uint8_t* scratch, int B, int Hin, int Win, int Hout,
                          int Wout, void* stream);
/* image_bgr / reference_bgr u8[B,H,W,3] (cv2 order), image_mask u8[B,H,W] = the blurred mask, mask_latent
 * u8[B,h,w] = the blurred mask resized to the latent grid.  Writes
 *   image            f32[B,3,H,W]  RGB planar: Image.composite(reference, image, image_mask) / 127.5 - 1
 *   cond_mask        f32[B,H,W]    round(image_mask / 255)
 *   cond_image       f32[B,3,H,W]  image * (1 - cond_mask)
 *   latmask          f32[B,4,h,w]  around(mask_latent / 255), tiled over the 4 latent channels
 *   cond_mask_latent f32[B,h,w]    nearest-neighbour resize of cond_mask (F.interpolate default) */
int ofx_sd_handoff(const uint8_t* image_bgr, const uint8_t* reference_bgr, const uint8_t* image_mask,
                   const uint8_t* mask_latent, float* image, float* cond_image, float* cond_mask, float* latmask,
                   float* cond_mask_latent, int B, int H, int W, int h, int w, void* stream);

/* ---------------------------------------------------------------- fill_mask_input (img2img_inpaint without a reference) */
/* PIL.ImageFilter.GaussianBlur(radius) on an interleaved 8-bit 4-channel image [B,H,W,4] ('RGBa' / 'RGBA': BoxBlur.c blurs the
 * four channels alike), bit-exact: the arithmetic of ofx_gaussian_blur_u8 per channel, but every row is prefix-summed in LDS, so
 * the cost does not depend on the radius.  in / out / scratch 4-byte aligned; scratch: B*H*W*4 bytes, distinct from in / out;
 * in == out is allowed; radius 0 is a copy.  max(H, W) <= 6144 (24 bytes of LDS per pixel of a row), B <= 65535 and
 * radius <= 65536: OFX_EINVAL beyond, before any launch. */
int ofx_gaussian_blur_rgba_u8(const uint8_t* in, uint8_t* out, uint8_t* scratch, int B, int H, int W, float radius,
                              void* stream);
/* fill_mask_input (guided_ldm_inpainting.py:161-176), bit-exact to Pillow: image_bgr u8[B,H,W,3] (the channel order does not
 * matter), mask u8[B,H,W] = the already blurred 'L' mask (255 = repaint) -> out_bgr u8[B,H,W,3], the frame with the masked
 * region filled from its surroundings: paste through 255 - mask onto an empty premultiplied canvas, then for (radius, repeats)
 * in (256,1) (64,1) (16,2) (4,4) (2,2) (0,1): GaussianBlur(radius), 'RGBa' -> 'RGBA', `repeats` alpha_composites onto the
 * accumulator; convert('RGB').  Where mask is 0 out is image exactly.  scratch: ofx_fill_mask_input_scratch_bytes(B, H, W)
 * bytes, 16-byte aligned, distinct from the three images.  The limits of ofx_gaussian_blur_rgba_u8 apply. */
size_t ofx_fill_mask_input_scratch_bytes(int B, int H, int W);
int ofx_fill_mask_input(const uint8_t* image_bgr, const uint8_t* mask, uint8_t* out_bgr, void* scratch, int B, int H, int W,
                        void* stream);

/* GroupNorm(groups, C, eps, affine) of an NHWC fp32 tensor [B,HW,C] (ldm/modules/diffusionmodules/model.py:40-41,
 * `Normalize` = 32 groups, eps 1e-6), optionally followed by x * sigmoid(x) (`nonlinearity`, :35-37): the pair in front
 * of every convolution of the VAE encoder.  gamma / beta: [C] or NULL.  Statistics in f64.  out may alias x.
 * scratch: ofx_groupnorm_scratch_bytes(B, C) bytes, 16-byte aligned.  B <= 65535 (OFX_EINVAL beyond: slice the batch). */
size_t ofx_groupnorm_scratch_bytes(int B, int C);
int ofx_groupnorm(const float* x, const float* gamma, const float* beta, float* out, void* scratch, size_t scratch_bytes,
                  int B, long HW, int C, int groups, float eps, int silu, void* stream);
/* in place: x[r][0..n) = softmax(x[r][0..n) * scale + bias[r % bias_rows][0..n)); columns n..ld-1 are set to 0 */
int ofx_softmax_rows(float* x, long rows, long ld, int n, float scale, const float* bias, long ld_bias, long bias_rows,
                     void* stream);
/* out[z] = softmax(q[z] k[z]^T * scale + bias) v[z] for z < BH; q [BH,Nq,D], k/v [BH,Nk,D], out [BH,Nq,D], fp32, D % 4 == 0.
 * The semantics of xformers.ops.memory_efficient_attention(q, k, v, attn_bias) (ldm/modules/attention.py:314,426) and of
 * AttnBlock.forward (model.py:179-203, BH = batch, D = channels).  bias: NULL, [Nq,Nk] shared by every z
 * (bias_bstride = 0) or [BH,Nq,Nk] (bias_bstride = Nq*Nk); -inf entries mask keys (a row with every key masked is NaN,
 * like softmax).  D in {40, 64, 80, 128, 160} (the UNet's head sizes) runs one fused kernel: online softmax, the scores
 * never leave the CU, ofx_attention_workspace_bytes() = 0 and `workspace` may be NULL.  Other D (the VAE's single
 * 512-wide head) run unfused: both GEMMs on the fp32 matrix cores, the score matrix in the workspace
 * (ofx_attention_workspace_bytes, 16-byte aligned; slice BH to bound it). */
size_t ofx_attention_workspace_bytes(int BH, int Nq, int Nk, int D);
int ofx_attention_f32(const float* q, const float* k, const float* v, const float* bias, long bias_bstride, float* out,
                      int BH, int Nq, int Nk, int D, float scale, void* workspace, size_t workspace_bytes, void* stream);
/* ofx_attention_f32 with the arithmetic of the two matrix products chosen by `precision` (an OFX_PREC_* value, defined below with
 * the convolutions' modes: 0 and 5 here).
 *   OFX_PREC_FP32 (0)  ofx_attention_f32 itself, bit for bit (called through).
 *   OFX_PREC_F16 (5)   opt-in, the fused head sizes D in {40, 64, 80, 128, 160} only -- any other D is OFX_EINVAL before any launch,
 *       there is no unfused fp16 path; no workspace.  q, k and v stay fp32 in memory; each element is rounded to fp16 once, to
 *       nearest even (v_cvt_pk_f16_f32), as it is staged; q is rounded UNSCALED.  Magnitudes beyond 65504 become infinities, as
 *       under torch.autocast; subnormals are not flushed.  K Q^T runs on v_mfma_f32_32x32x16_f16 with fp32 accumulation (D = 40 as
 *       48 with zero pad columns); the logit is fma(score, scale * log2 e, bias * log2 e) in fp32, so neither the scale nor the bias
 *       passes through fp16.  The maximum, v_exp_f32, the running sum l (summed from the fp32 probabilities BEFORE they are
 *       rounded), the O accumulators, the rescale and 1 / l are fp32.  P is rounded to fp16 (nearest even) for P V, also with fp32
 *       accumulation.  Error on top of the fp32 kernel's: the operand roundings (2^-11 relative each; the tests compare against
 *       float64 on the rounded operands, where they vanish) and 2^-11 sum_j p_j |v_jd| + 2^-25 sum_j |v_jd| for the rounding of P.
 *   any other value    OFX_EINVAL before any launch. */
int ofx_attention_prec(const float* q, const float* k, const float* v, const float* bias, long bias_bstride, float* out,
                       int BH, int Nq, int Nk, int D, float scale, int precision, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---------------------------------------------------------------- SpatialTransformer (ldm/modules/attention.py:472-537) */
/* nn.LayerNorm(C) over the last axis of `rows` rows (BasicTransformerBlock.norm1 / norm2 / norm3, attention.py:456-458, applied at
 * :465-468): out[r][c] = (x[r][c] - mean_r) / sqrt(var_r + eps) * gamma[c] + beta[c], var biased, eps a parameter (the reference's
 * nn.LayerNorm default is 1e-5).  Rows are ldx / ldo floats apart (ld >= C, ld % 4 == 0: a last-axis slice of a wider tensor is a
 * valid operand); gamma / beta: [C] or NULL.  C % 4 == 0, C <= 4096 (OFX_EINVAL beyond), pointers 16-byte aligned (OFX_EALIGN).
 * out == x is allowed.  One wave per row with the row in registers: the mean first, then the sum of squares of the centred values,
 * both by wave reductions; no LDS, no scratch. */
int ofx_layernorm(const float* x, int ldx, const float* gamma, const float* beta, float* out, int ldo, int rows, int C, float eps,
                  void* stream);
/* GEGLU.forward after its Linear (attention.py:54-56: `x, gate = self.proj(x).chunk(2, dim=-1); return x * F.gelu(gate)`):
 * out[r][c] = a[r][c] * gelu(a[r][inner + c]) for c < inner, gelu(g) = g/2 * (1 + erf(g / sqrt 2)), the exact form F.gelu defaults
 * to.  Rows of a are lda >= 2 * inner floats apart, rows of out ldo >= inner; inner, lda, ldo % 4 == 0, 16-byte aligned. */
int ofx_geglu(const float* a, int lda, float* out, int ldo, int rows, int inner, void* stream);
/* ofx_attention_f32 on token rows (MemoryEfficientCrossAttention.forward, attention.py:326-436, without its permute + contiguous
 * copies at :338-345 and :430-435): element (b, n, h, d) of q / k / v / out lives at p[(b * N + n) * ld + h * D + d], N = Nq for q
 * and out, Nk for k and v -- tokens are rows, the heads sit side by side in a row.  The four strides are independent, each
 * >= H * D and % 4 == 0, so one [B, N, 3 * H * D] buffer of a fused q|k|v projection is three valid operands with ld = 3 * H * D.
 * bias: NULL, [Nq,Nk] shared (bias_bstride = 0) or [B*H,Nq,Nk] (bias_bstride = Nq*Nk), batch-head z = b * H + h.  Only the head
 * sizes of the fused kernel, D in {40, 64, 80, 128, 160}; any other D is OFX_EINVAL (permute and call ofx_attention_f32).  The
 * same kernel with other addresses: bit-identical to ofx_attention_f32 on the permuted contiguous copies.  No workspace. */
int ofx_attention_bnhd_f32(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* bias,
                           long bias_bstride, float* out, int ldo, int B, int H, int Nq, int Nk, int D, float scale, void* stream);
/* ofx_attention_bnhd_f32 with `precision` as in ofx_attention_prec: OFX_PREC_FP32 calls through, bit for bit; OFX_PREC_F16 is the fp16
 * matrix-core kernel on the same addresses (bit-identical to ofx_attention_prec on the permuted contiguous copies); any other
 * value is OFX_EINVAL before any launch.  The argument checks of ofx_attention_bnhd_f32 apply unchanged. */
int ofx_attention_bnhd_prec(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* bias,
                            long bias_bstride, float* out, int ldo, int B, int H, int Nq, int Nk, int D, float scale, int precision,
                            void* stream);
/* ofx_attention_bnhd_prec with K and V read through a segment table, in place: K / V of image b are the logical concatenation of
 * seg_counts[b] segments -- what torch.cat along the tokens would build -- and image b owns the next seg_counts[b] entries of
 * `segs` (a HOST array of sum(seg_counts) entries, copied into the kernel arguments: no device allocation, nothing to keep alive
 * after the call returns but the tensors themselves).  A segment is n tokens; token t of it has head h at k[t * ldk + h * D],
 * v[t * ldv + h * D] (strides in elements).  kv_type is the element type of EVERY segment of the launch: OFX_KV_F32, or OFX_KV_F16
 * (IEEE half) -- half elements feed the OFX_PREC_F16 kernel as they are (no second rounding) and are converted exactly in the
 * OFX_PREC_FP32 kernel.  q, bias and out are float32 as in ofx_attention_bnhd_f32; Nk is the per-image total.  The tile walk, the
 * bias column, the ragged-tail mask and the online softmax use the logical key index, so the result is bit for bit that of
 * ofx_attention_bnhd_prec on the concatenated float32 tensors (for OFX_KV_F16: on the halves widened to float32, and with
 * OFX_PREC_F16 also on any float32 values that round to those halves).
 * OFX_EINVAL before any launch: D outside {40, 64, 80, 128, 160}; seg_counts[b] outside 1 .. OFX_KV_MAX_SEGMENTS; more than
 * OFX_KV_MAX_ENTRIES entries in all; n <= 0; per-image totals that differ; a segment with a null or misaligned pointer (16 bytes
 * for float32 rows, 8 for half rows), a stride < H * D or not a multiple of 4 elements; an unknown kv_type or precision.  q, bias
 * and out are checked as ofx_attention_bnhd_f32 checks them (OFX_EALIGN for their alignment). */
#define OFX_KV_F32 0
#define OFX_KV_F16 1
#define OFX_KV_MAX_SEGMENTS 8
#define OFX_KV_MAX_ENTRIES 64
typedef struct ofx_kv_segment {
    const void* k;   /* n rows of keys,   ldk elements apart */
    const void* v;   /* n rows of values, ldv elements apart */
    int n;
    int ldk;
    int ldv;
} ofx_kv_segment;
int ofx_attention_bnhd_segs(const float* q, int ldq, const ofx_kv_segment* segs, const int* seg_counts, int kv_type, const float* bias,
                            long bias_bstride, float* out, int ldo, int B, int H, int Nq, int D, float scale, int precision,
                            void* stream);

/* ---------------------------------------------------------------- first-stage decoder (decode_first_stage / decode_latent) */
/* `Upsample` of the VAE decoder (ldm/modules/diffusionmodules/model.py:43-58): out = conv3x3(pad 1)(interpolate(x, 2x, nearest)) + bias
 * without materialising the upsampled map.  Output pixel (2y + py, 2x + px) only sees the 2x2 low-resolution neighbourhood
 * {y - 1 + py, y + py} x {x - 1 + px, x + px}: four 2x2 convolutions (one per parity) with the 3x3 taps that fall on the same
 * low-resolution pixel added up beforehand -- 4 multiplies per output instead of 9; the zero padding of the upsampled map coincides
 * with zero padding of the low-resolution map.
 * ofx_upconv2x_weight (host): OIHW fp32 3x3 weights -> the four folded operands, summed in float64 and rounded once, as
 * [4 parities][Cout][4 taps][Cin] floats (the exact index is documented at the definition, vae_dec.hip).  Returns the float count
 * 16 * Cout * Cin (`out` may be NULL to query it) or OFX_EINVAL.
 * ofx_upconv2x: x NHWC fp32 [B,H,W,Cin] (dense), w from ofx_upconv2x_weight (device), bias [Cout] or NULL -> out[((b*2H + Y)*2W + X)*ldo + n],
 * ldo >= Cout, on v_mfma_f32_32x32x2_f32.  Any H, W >= 1 and any Cout; Cin % 4 == 0 and x, w 16-byte aligned (OFX_EALIGN otherwise);
 * B*2H*2W < 2^31 (OFX_EINVAL beyond: slice the batch; addresses themselves are 64-bit). */
long ofx_upconv2x_weight(const float* w_oihw, int Cout, int Cin, float* out);
int ofx_upconv2x(const float* x, const float* w, const float* bias, float* out, int ldo, int B, int H, int W, int Cin, int Cout,
                 void* stream);
/* ofx_upconv2x with the arithmetic of the contraction chosen by `precision` (an OFX_PREC_* value, defined below with the convolutions'
 * modes: 0, 5 and 7 here).  The argument checks of ofx_upconv2x apply unchanged.
 *   OFX_PREC_FP32 (0)  ofx_upconv2x itself, bit for bit (called through).
 *   OFX_PREC_F16 (5)   opt-in (`VaeDecoder(precision="fp16")`): the arithmetic of OFX_PREC_F16 in ofx_conv2d on the same four parity
 *       GEMMs and the same 128 x BN tiles.  x and the folded w stay fp32 in memory; each element is rounded to fp16 once, to nearest
 *       even (v_cvt_pk_f16_f32), as it is staged, 32 channels of a tap per chunk; one v_mfma_f32_32x32x16_f16 per 16 k with fp32
 *       accumulation; the bias add and the stored result are fp32.  It is the FOLDED weight that is rounded (w1 + w2 summed in
 *       float64, rounded to fp32 by ofx_upconv2x_weight, then to fp16 here), so the result differs from the unfused fp16 pair by
 *       those roundings.  Magnitudes beyond 65504 become infinities, as under torch.autocast; subnormals are not flushed.
 *   OFX_PREC_F16_W (7) the kernel of OFX_PREC_F16 with `w` read as IEEE halves [4][Cout][4][Cin] (ofx_half_conv_weight of the folded
 *       fp32 operand; 16-byte aligned): staged as they are, bit-identical to 5 on fp32 weights that round to them.  ofx_upconv2x_bn
 *       answers as for 5.
 *   any other value   OFX_EINVAL before any launch.
 * ofx_upconv2x_bn (host, no device): the column-tile width BN in {64, 128} of the 128 x BN tile both entry points launch for this
 * Cout and precision (OFX_EINVAL for Cout <= 0 or another precision). */
int ofx_upconv2x_prec(const float* x, const float* w, const float* bias, float* out, int ldo, int B, int H, int W, int Cin, int Cout,
                      int precision, void* stream);
int ofx_upconv2x_bn(int Cout, int precision);
/* F.interpolate(x, scale_factor=2.0, mode="nearest") of an NHWC fp32 tensor: [B,H,W,C] -> [B,2H,2W,C] (the materialising half of the
 * unfused pair; the VAE decoder takes it with OFX_VAE_NO_UPCONV=1).  C % 4 == 0, 16-byte aligned; B*2H*2W < 2^31. */
int ofx_upsample2x_nearest_f32(const float* in, float* out, int B, int H, int W, int C, void* stream);
/* decode_latent's exit (ofgen_keyframe_inpaint.py:234-235): x f32 NHWC RGB rows of ld >= 3 floats -> out u8 BGR [B,H,W,3] =
 * (clip(x, -1, 1) * 127.5 + 127.5) truncated toward zero, the product and the sum rounded separately in fp32 (numpy's bits).
 * x and out 4-byte aligned. */
int ofx_decode_to_u8(const float* x, int ld, uint8_t* out, int B, int H, int W, void* stream);

/* ---------------------------------------------------------------- UNet (ldm/modules/diffusionmodules/openaimodel.py:415-793) */
/* GroupNorm over a channel concatenation with a per-image, per-channel term folded in: what `ResBlock._forward` needs twice
 * (openaimodel.py:257-277).  `in_layers` of an output block normalises th.cat([h, hs.pop()], dim=1) (:786, groups straddle the
 * seam: 1280 + 640 channels are 60 per group), `out_layers` normalises h + emb_out[b, c] (:275-276):
 *   out[b][p][c] = act(GN_groups(cat(x0, x1)[b][p][:] + e[b][:])[c] * gamma[c] + beta[c]),   act = x * sigmoid(x) when silu
 * x0 [B,HW,C0] with rows ld0 floats apart, x1 [B,HW,C1] with rows ld1 apart or NULL with C1 = 0, e [B][C0 + C1] with rows lde
 * apart or NULL (a slice of one buffer that holds every emb projection is a valid operand), gamma / beta [C0 + C1] or NULL, out
 * dense [B,HW,C0 + C1].  C0, C1, ld0, ld1 % 4 == 0 and x0, x1, e, out, scratch 16-byte aligned (OFX_EALIGN); (C0 + C1) % groups
 * == 0, ld0 >= C0, ld1 >= C1, lde >= C0 + C1, B <= 65535 (OFX_EINVAL).  out may alias x0 only when C1 = 0 and ld0 = C0; any other
 * overlap of out with x0 or x1 is OFX_EINVAL.  The three stages and the summation order of ofx_groupnorm (per-channel f64 sums
 * S_c, Q_c per image slice, one workgroup per image, a float4 apply); e enters in the second stage only, in f64: the sums of
 * x + e over n pixels are S_c + n e and Q_c + 2 e S_c + n e^2, and (x + e) * scale + shift = x * scale + (shift + e * scale), so
 * the shifted map is never written.  With C1 = 0, ld0 = C0 and e = NULL the result is bit-identical to ofx_groupnorm.
 * scratch: ofx_groupnorm_cat_scratch_bytes(B, C0 + C1) bytes. */
size_t ofx_groupnorm_cat_scratch_bytes(int B, int C);
int ofx_groupnorm_cat(const float* x0, int ld0, int C0, const float* x1, int ld1, int C1, const float* e, int lde,
                      const float* gamma, const float* beta, float* out, void* scratch, size_t scratch_bytes, int B, long HW,
                      int groups, float eps, int silu, void* stream);
/* The Linear layers of the timestep path on a handful of rows (`time_embed`, openaimodel.py:530-534, and `emb_layers` of every
 * ResBlock, :220-226, applied at :266 and :771):  out[b][n] = sum_k s(x[b][k]) * w[n][k] + bias[n],  s = x * sigmoid(x) when silu_in
 * (the nn.SiLU in front of the Linear), the identity otherwise.  x [B][K] with rows ldx apart, w the checkpoint's own row-major
 * [N][K] (not packed), bias [N] or NULL, out rows ldo >= N apart (columns N..ldo-1 are not touched).  B <= 16 (OFX_EINVAL beyond:
 * slice the rows); K, ldx % 4 == 0 and x, w 16-byte aligned (OFX_EALIGN); any N.  The rows go to LDS once (SiLU on the way in), one
 * wave per output column reads its weight row with float4 loads and reduces across the wave in a fixed order: weight-read bound,
 * no matrix cores. */
int ofx_emb_linear(const float* x, int ldx, const float* w, const float* bias, float* out, int ldo, int B, int K, int N, int silu_in,
                   void* stream);
/* `timestep_embedding` (ldm/modules/diffusionmodules/util.py:154-174, repeat_only=False): out[b][j] = cos(t[b] * freqs[j]) and
 * out[b][half + j] = sin(t[b] * freqs[j]) for j < half = dim / 2; an odd dim gets a zero last column (:170-171).  t [B] fp32 on the
 * device (fractional timesteps are legal), freqs [half] fp32 on the device: the table the reference builds on the CPU and moves
 * (:165-167).  out dense [B][dim].  The product is one fp32 multiplication, sinf / cosf the accurate ones (arguments reach 1e3). */
int ofx_timestep_embedding(const float* t, const float* freqs, float* out, int B, int dim, void* stream);

/* ---------------------------------------------------------------- ControlNet (controlnet.py:65-322) */
/* One layer of `input_hint_block` (controlnet.py:164-180): a 3x3 convolution, padding 1, stride 1 or 2, with bias and nn.SiLU in
 * the epilogue:   y = sum_{ky,kx,c} x[b][oy*stride - 1 + ky][ox*stride - 1 + kx][c] * w[n][(ky*3 + kx)*Cin + c] + bias[n],
 *   out[((b*Hout + oy)*Wout + ox)*ldo + n] = silu ? y * sigmoid(y) : y,      Hout = (H - 1)/stride + 1, Wout = (W - 1)/stride + 1
 * x NHWC fp32 [B,H,W,Cin] with pixel rows ldx floats apart, taps outside the image read zeros; w is ofx_pack_conv_weight's operand
 * with cin_pad = Cin, rows ldw >= 9*Cin floats apart (its Kpad); a 3-channel hint is padded to Cin = 4 with zero weights.  bias
 * [Cout] or NULL.  Only columns [0, Cout) of an output row are written.  Exact fp32 on v_mfma_f32_16x16x4_f32 (output pixels on
 * the M side, 16 channels on the N side, so Cout = 16 fills the instruction), the halo patch and the weights through LDS.  The
 * sum runs in (channel chunk, ky, kx, channel) order on two levels: a fused multiply-add chain per chunk of 8 channels (4 when
 * Cin % 8 != 0), the chunk sums added in order.  The sigmoid is the one of ofx_groupnorm's SiLU.  Checked before any launch: OFX_EINVAL for a NULL x / w / out, a stride other than 1 or 2, a non-positive
 * size, Cin % 4 != 0, Cout % 16 != 0, ldx < Cin, ldo < Cout, ldw < 9*Cin, B*H*W >= 2^31 (slice the batch; addresses themselves
 * are 64-bit); OFX_EALIGN for ldx, ldo or ldw % 4 != 0 or x, w, out not 16-byte aligned. */
int ofx_conv3x3_silu(const float* x, int ldx, int Cin, const float* w, int ldw, const float* bias, float* out, int ldo, int Cout,
                     int B, int H, int W, int stride, int silu, void* stream);

/* ---------------------------------------------------------------- CLIP text encoder (hack.py:32-70, FrozenCLIPEmbedder) */
/* CLIPTextEmbeddings.forward, the entry of the text transformer `_hacked_clip_forward` feeds its 77-token chunks to (hack.py:42-47,
 * :66-67):   out[r][c] = tok[ids[r]][c] + pos[r % T][c],   r < rows, c < C     (one fp32 addition, so bit-identical to torch's)
 * ids [rows] int32 on the device (the reference feeds torch.IntTensor, hack.py:64), rows = sequences * T in sequence-major order;
 * tok [vocab][C] and pos [>= T][C], the checkpoint's own row-major token_embedding / position_embedding tensors, not packed; out
 * rows ldo >= C floats apart, columns C..ldo-1 are not touched.  An id outside [0, vocab) reads nothing: its output row is all
 * quiet NaN and every other row is unaffected (no clamp).  OFX_EINVAL for a NULL pointer, rows < 0, T, C or vocab <= 0, ldo < C;
 * OFX_EALIGN for C or ldo % 4 != 0, tok, pos or out not 16-byte aligned, ids not 4-byte aligned; all before any HIP call.
 * rows == 0 is a successful no-op.  One float4 per lane per trip, a wave on 64 consecutive float4 of a row (256-float runs of
 * both tables and of the output), grid-stride over rows * C / 4 with 64-bit indices: any row count, at most 65536 workgroups. */
int ofx_clip_embed(const int32_t* ids, const float* tok, const float* pos, float* out, int ldo, long rows, int T, int C, int vocab,
                   void* stream);
/* quick_gelu over token rows, the activation of CLIPMLP (hidden_act "quick_gelu", what FrozenCLIPEmbedder's checkpoint is):
 *   out[r][c] = x[r][c] * sigmoid(1.702f * x[r][c]),   c < n,   evaluated as x / (1 + expf(-(1.702f * x))) in fp32 with the accurate
 * expf and an IEEE division.  Finite for every finite x: where the exponential overflows (x < -52.1) the quotient is -0.  Rows of
 * x / out are ldx / ldo >= n floats apart (a last-axis slice is a valid operand), columns n.. are not touched; out == x is allowed.
 * OFX_EINVAL for a NULL pointer, rows < 0, n <= 0, ldx < n or ldo < n; OFX_EALIGN for n, ldx or ldo % 4 != 0 or a pointer not
 * 16-byte aligned; all before any HIP call.  rows == 0 is a successful no-op.  The same one-float4-per-lane grid-stride loop. */
int ofx_quick_gelu(const float* x, int ldx, float* out, int ldo, long rows, int n, void* stream);

/* ---------------------------------------------------------------- sampler (guided_ldm_inpainting.py:28-137, guided_ldm.py:30-158) */
/* The scalars of one DDIM step, fp32 as the reference forms them: cfg = unconditional_guidance_scale, sqrt_at = sqrt(ddim_alphas
 * [index]), sqrt_1m_at = ddim_sqrt_one_minus_alphas[index], sqrt_aprev = sqrt(ddim_alphas_prev[index]), dir_coef = sqrt(1 - a_prev -
 * sigma_t^2), sigma_t = ddim_sigmas[index] * temperature, g = the scalar guidance strength, sa / s1 = sqrt_alphas_cumprod /
 * sqrt_one_minus_alphas_cumprod at the DDPM timestep of the NEXT step (what its q_sample reads). */
typedef struct ofx_ddim_coef {
    float cfg, sqrt_at, sqrt_1m_at, sqrt_aprev, dir_coef, sigma_t, g, sa, s1;
} ofx_ddim_coef;
#define OFX_DDIM_STEP       0   /* the whole chain below */
#define OFX_DDIM_BLEND_ONLY 1   /* xp = x, then the blend: the blend before the first step and img2img_inpaint's final one */
/* One guided DDIM step and the mask blend that opens the next one, per pixel row of C floats (C % 4 == 0), in this order:
 *   e    = eps_u + cfg * (eps_c - eps_u)                       eps_u NULL: e = eps_c (no classifier-free guidance)
 *   pred = (x - sqrt_1m_at * e) / sqrt_at
 *   with guidance:  pred = pred * (1 - g) + guidance * g       g = gmap[row] when gmap is given, coef->g otherwise
 *                   e    = (x - sqrt_at * pred) / sqrt_1m_at
 *   xp   = sqrt_aprev * pred + dir_coef * e  [+ sigma_t * step_noise]
 *   with nmask:     xp = (1 - nmask) * (sa * init + s1 * blend_noise) + nmask * xp      blend_noise NULL needs s1 == 0
 *   out0[row] = xp;   out1[row] = xp when given;   pred_out[row] = pred when given
 * OFX_DDIM_BLEND_ONLY skips everything above the blend (xp = x): eps_c, eps_u, guidance, gmap, step_noise and pred_out must be
 * NULL and nmask given.  Every tensor is [rows][C] with its rows ld* floats apart (eps_c and eps_u share lde), so a channel slice of
 * a wider NHWC buffer is a valid operand: out0 / out1 are meant to be channels 0..C-1 of the two halves of the UNet's padded
 * input, and only those C floats of a row are written.  gmap is [rows].  ld* % 4 == 0, C % 4 == 0 and 16-byte aligned pointers
 * (OFX_EALIGN); NULL x / out0 / coef (eps_c in OFX_DDIM_STEP), init without nmask or the reverse, gmap without guidance, ld < C,
 * rows <= 0, an unknown mode (OFX_EINVAL).  out0 and out1 may each be exactly x (same pointer and row stride: a thread reads its
 * float4 of every operand before it writes); any other overlap between an output and an input or between two outputs is
 * OFX_EINVAL.  All of this is checked before the launch. */
int ofx_ddim_step(const float* x, int ldx, const float* eps_c, const float* eps_u, int lde, const float* guidance, int ldg,
                  const float* gmap, const float* step_noise, int ldsn, const float* init, int ldi, const float* nmask, int ldm,
                  const float* blend_noise, int ldbn, float* out0, int ldo0, float* out1, int ldo1, float* pred_out, int ldp,
                  const ofx_ddim_coef* coef, int mode, long rows, int C, void* stream);

/* ---------------------------------------------------------------- key-frame detector */
/* edges[b] = cv2.dilate(cv2.Canny(V, low, high), ones(ksize, ksize)) for BGR frames u8[B,H,W,3], with V = max(B,G,R)
 * (the HSV value channel) and low/high = int((1 -/+ 1/3) * np.median(V)) clipped to [0,255]
 * (_detect_edges, ofgen_keyframe_inpaint.py:161-192).  ksize odd (estimated_kernel_size, :153-158).
 * scratch: ofx_detect_edges_scratch_bytes(B,H,W) bytes, 256-byte aligned.  The hysteresis stage iterates to
 * convergence and SYNCHRONISES the stream once per batch of 8 sweeps (the only blocking call of the library).  Parity: OpenCV's algorithm restated; unpinned. */
size_t ofx_detect_edges_scratch_bytes(int B, int H, int W);
int ofx_detect_edges(const uint8_t* frames_bgr, uint8_t* edges, void* scratch, size_t scratch_bytes, int B, int H,
                     int W, int ksize, void* stream);
/* edges[b] = cv2.Canny(images[b], low, high) (aperture 3, L2gradient=false) for u8 [B,H,W] (channels 1) or [B,H,W,3]
 * (channels 3) images: what ControlNet's 'canny' detector computes (extract_control, controlnet.py:343-347).  The 3x3 Sobel
 * runs per channel and a pixel keeps the (dx, dy, |dx|+|dy|) of the channel with the largest norm, the lowest channel on a
 * tie; then the suppression and hysteresis stages of ofx_detect_edges (they are shared), m > low a candidate, m > high
 * strong; low > high are swapped.  edges: u8 [B,H,W], 255 or 0, no dilation.  scratch: ofx_canny_u8_scratch_bytes(B,H,W)
 * bytes, 256-byte aligned; like ofx_detect_edges the call SYNCHRONISES the stream once per batch of 8 sweeps.  Checked
 * before any launch: NULL pointers, channels not 1 or 3, B outside 1..65535, H or W <= 0 (OFX_EINVAL), a misaligned
 * (OFX_EALIGN) or too small (OFX_ENOMEM) scratch.  Parity: OpenCV's algorithm restated; unpinned. */
size_t ofx_canny_u8_scratch_bytes(int B, int H, int W);
int ofx_canny_u8(const uint8_t* images, int channels, uint8_t* edges, void* scratch, size_t scratch_bytes, int B, int H,
                 int W, int low, int high, void* stream);
/* sums[b] = sum_i |a[b*a_bstride + i] - b_[b*b_bstride + i]|, i < n (mean_pixel_distance's numerator, :143-150);
 * a stride of 0 compares every image with one shared image.  sums: device u64[B]. */
int ofx_abs_diff_sum_u8(const uint8_t* a, long a_bstride, const uint8_t* b, long b_bstride,
                        unsigned long long* sums, int B, long n, void* stream);

/* ---------------------------------------------------------------- implicit-GEMM conv */
#define OFX_ACT_NONE    0   /* max(v, -FLT_MAX): finite sums pass unchanged, a NaN or -inf sum comes out as -FLT_MAX (the plain epilogue does not propagate NaN) */
#define OFX_ACT_RELU    1
#define OFX_ACT_SIGMOID 2
#define OFX_ACT_TANH    3

#define OFX_EPI_PLAIN   0   /* y = act(acc*scale + shift); if res: y = relu(y + res)            */
#define OFX_EPI_GRU_ZR  1   /* Cout=2*hd: n<hd -> z=sigmoid -> aux_z ; n>=hd -> r -> aux_rh=r*h.  hd % 32 == 0 (else OFX_EINVAL: the
                               kernels take z or r per 32-column sub-tile).  aux_z and aux_rh are dense [M][hd] rows of hd floats:
                               aux_z[m*hd + n], aux_rh[m*hd + n - hd] = r * aux_h[m*ldh + n - hd]; aux_h is only read, ldh >= hd */
#define OFX_EPI_GRU_Q   2   /* q=tanh; h = (1-z)*h + z*q written in place to aux_h[m*ldh + n], n < Cout = hd, ldh >= Cout; z is
                               read from aux_z[m*Cout + n]: dense rows of Cout floats, the array GRU_ZR wrote */
#define OFX_EPI_FLOW    3   /* Cout=2: coords1 += delta; flow=coords1-grid -> aux_h slot + flow4.  The generic form of the flow
                               head's second convolution; the RAFT executor itself runs flow_head.hip, which leaves convf1's
                               operand as 16-float flow rows instead of this [M][4] array */

/* Arithmetic of the matrix-core contractions.  FP32 is the reference's (and the default): v_mfma_f32_32x32x2_f32,
 * bit-identical to an fmaf chain.  BF16X3 is an opt-in fast mode: each fp32 operand is split on the fly into
 * hi = bf16(x), lo = bf16(x - hi) and the product is formed as hi*hi + hi*lo + lo*hi on the bf16 matrix cores
 * with fp32 accumulation (operands carry ~16 mantissa bits; measured end-to-end flow EPE ~1e-4 px). */
#define OFX_PREC_FP32   0
#define OFX_PREC_BF16X3 1
#define OFX_PREC_BF16X3_W 2   /* bf16x3 with `w` already in the split format of ofx_split_conv_weight */
#define OFX_PREC_BF16X6_W 4   /* bf16x6 with `w` already in the split format of ofx_split_conv_weight3 */
#define OFX_PREC_BF16X6 3     /* opt-in: fp32 operands split into THREE bf16 pieces (exact), the six products of weight >= 2^-16
                                 on the bf16 matrix cores, fp32 accumulate: fp32-level accuracy (dropped terms < 2^-23), not the
                                 bit pattern of an fmaf chain */
#define OFX_PREC_F16 5        /* opt-in: both operands rounded fp32 -> fp16 (round-to-nearest-even) as they are staged, ONE product per
                                 operand pair on v_mfma_f32_32x32x16_f16, fp32 accumulate -- the arithmetic torch.autocast gives the
                                 reference's diffusion stage.  Activations, weights ([Cout][Kpad] fp32, converted in the kernel) and
                                 the epilogue stay fp32.  Error: 2^-11 relative per operand, i.e. ~2^-10 * sum |x||w| per output.
                                 Range: an operand beyond +-65504 becomes an infinity, as the convert instruction makes it and as
                                 autocast does (the result is then inf / NaN; the identity epilogue stores +-FLT_MAX for them).
                                 Subnormals: operands below 2^-14 in magnitude become fp16 subnormals (multiples of 2^-24) and
                                 the matrix core multiplies them as such -- nothing is flushed (held by the small-magnitude case
                                 of tests/f16_check.py; were they flushed, that case's bound would need the extra term
                                 K * 2^-14 * max |other operand|).
                                 Serves the plain epilogue only (identity / ReLU / sigmoid / tanh with scale, shift, addend, res,
                                 two segments, out / ldo, stride), tiles 128x128, 128x64 and 64x64, BK 16 or 32, the halo-patch
                                 schedule included.  OFX_EINVAL, from ofx_conv2d and ofx_conv2d_plan alike and before any launch:
                                 the GRU / flow epilogues, nmean / nrstd, ofx_conv2d_stats, nz > 1, the pooled correlation
                                 volume, a split-K workspace (splitk_ws != NULL) and the paired-pipeline tile marker.  wino_w /
                                 wino4_w are ignored, as under the split-bf16 modes */
#define OFX_PREC_F16_EPI (OFX_PREC_F16 | 256)   /* 261: the arithmetic, tiles and kernels of OFX_PREC_F16 (ofx_conv_plan.prec reads
                                 OFX_PREC_F16) with three more things served, the descriptors of the flow network under
                                 OFX_RAFT_F16: the GRU gate epilogues OFX_EPI_GRU_ZR / _Q (the gate algebra is fp32 on the
                                 accumulators); nmean / nrstd (the normalised, ReLU'd fp32 value is what is rounded to half);
                                 ofx_conv2d_stats (the statistics come from the fp32 accumulators, as in fp32).  A value of its own so
                                 that what OFX_PREC_F16 documents as rejected stays rejected for callers written against it.  Still
                                 OFX_EINVAL before any launch: the flow epilogue, nz > 1, the pooled volume, a split-K workspace
                                 and the paired-pipeline tile marker */
#define OFX_PREC_F16_W 7      /* OFX_PREC_F16 with `w` already in the kernel's format: IEEE halves [Cout][Kpad] (same packing, k order
                                 and Kpad; rows are multiples of 64 bytes, `w` 16-byte aligned), as ofx_half_conv_weight makes them from
                                 the packed fp32 matrix.  The halves are staged as they are -- no convert, no second rounding -- so the
                                 output is bit-identical to OFX_PREC_F16 on any fp32 weights that round to them, at half the weight
                                 bytes held and streamed.  The arithmetic, tiles, schedules, plain epilogue, plan (every field but
                                 `prec`, which reads OFX_PREC_F16_W) and rejections of OFX_PREC_F16; the extensions of
                                 OFX_PREC_F16_EPI do not exist in this format (7 | 256 is OFX_EINVAL) */

typedef struct ofx_conv_desc {
    /* input: NHWC fp32, up to two channel segments (torch.cat along C without materialising) */
    const float* in0; int ld0; int c0;
    const float* in1; int ld1; int c1;          /* in1 may be NULL (c1 = 0); with in1, c0 and c1 multiples of 32 (else OFX_EALIGN) */
    /* weights packed [Cout][Kpad], k = (ky*KW + kx)*(c0+c1) + c, Kpad = K rounded up to 32.  fp32, except under the `_W` precisions,
       which read the field in their own format: OFX_PREC_F16_W reads it as IEEE halves [Cout][Kpad] (2 bytes per element) */
    const float* w;
    const float* scale;                          /* [Cout] or NULL (=1) */
    const float* shift;                          /* [Cout] or NULL (=0) */
    float* out; int ldo;                         /* out[m*ldo + n]; may be NULL for GRU/FLOW epilogues */
    const float* res; int ldres;                 /* residual for EPI_PLAIN, or NULL */
    const float* nmean; const float* nrstd;      /* instance-norm(+ReLU) applied to in0 on load, [B][c0], or NULL */
    const float* addend; int ldadd;              /* optional pre-activation term: v += addend[m*ldadd + n]       */
    float* aux_z; float* aux_rh; float* aux_h; int ldh;   /* GRU buffers; hidden dim = Cout(Q) */
    float* aux_coords; float* aux_flow4;         /* EPI_FLOW only: coords1 [M][2], flow4 [M][4] = (fx, fy, 0, 0) per pixel */
    long a_zs, w_zs, o_zs; int nz;               /* batched-GEMM mode (nz>1): per-z strides in elements */
    int B, Hin, Win, Hout, Wout, Cout, KH, KW, stride, padH, padW;
                                                 /* Geometry: out[b, oy, ox, n] sums x[b, oy*stride - padH + ky, ox*stride - padW + kx, c]
                                                    * w[n][(ky*KW + kx)*(c0+c1) + c] over ky < KH, kx < KW, c; a tap outside
                                                    [0, Hin) x [0, Win) contributes zero (never the next row or image), also under
                                                    nmean / nrstd.  padH, padW >= 0 (negative: OFX_EINVAL) are the rows above and the
                                                    columns left of the image; Hout and Wout are the caller's: any positive size, smaller
                                                    or larger than (Hin + 2 padH - KH) / stride + 1 (outputs beyond it read zeros below
                                                    and to the right; padH = padW = 0, stride 2, Hout = Hin / 2 is the VAE's Downsample).
                                                    The direct kernels' general and scalar-coordinate schedules serve every such
                                                    descriptor; the halo-patch schedule and the Winograd routes take only 'same' stride-1
                                                    ones (padH = KH / 2, padW = KW / 2, Hout = Hin, Wout = Win): any other is planned
                                                    on the former, and a tile that forces a Winograd route for it is OFX_EINVAL */
    int act, epi;
    int tile;                                    /* 0 = auto; else [2000000000 +] BK*1000000 + BM*1000 + BN, e.g. 16128128;
                                                    tiles 128x{32,64,128,192}, 64x64; BK 16 or 32; the 2e9 marker selects the
                                                    paired-pipeline variant of the 64x64 / BK 32 tile (small grids).  fp32: a BK
                                                    or a marker the BM x BN tile does not exist with is OFX_EINVAL (BK may be
                                                    left out: BM*1000 + BN takes the tile's own) */
    int precision;                               /* OFX_PREC_FP32 (default, exact fp32 MFMA) or one of the opt-in OFX_PREC_* above */
    void* splitk_ws;                             /* optional device scratch (256-byte aligned) for split-K on small grids: */
    size_t splitk_ws_bytes;                      /* partial tiles + per-tile arrival counters.  The first 64 KiB hold the
                                                    counters and must be ZERO before the first use (the kernel leaves them
                                                    zero); one scratch per stream that may run a convolution concurrently.
                                                    NULL / 0: never split. */
    const float* wino_w;                         /* optional (3x3 layers): the same weights as ofx_wino_conv_weight makes them.
                                                    When set, a layer runs the fused Winograd F(2x2,3x3) kernel on grids that
                                                    fill the chip if all of these hold:
                                                    - fp32, stride 1, 'same' padding, a map of whole 8x16 patches;
                                                    - plain epilogue, ReLU or identity, no addend;
                                                    - `res` (residual merge) is allowed;
                                                    - a fused norm (`nmean` / `nrstd`) is allowed over a single input segment;
                                                    - under ofx_conv2d_stats, only identity outputs without `res` qualify, and
                                                      the partials come one row per 8x16 patch.
                                                    Otherwise, or with OFX_CONV_NO_WINOGRAD in the
                                                    environment, the direct kernels run.  tile = OFX_CONV_TILE_WINOGRAD
                                                    forces it at any grid size and is rejected (OFX_EINVAL) when the layer does not
                                                    qualify.  NULL: direct kernels only.
                                                    1x5 / 5x1 layers: the operand of ofx_wino15_conv_weight.  A stride-1 fp32
                                                    layer keeping the map size (pad 0,2 / 2,0) over whole 8x16 patches, with a
                                                    plain (ReLU / identity, optional addend) or GRU gate epilogue, runs the fused
                                                    1D Winograd F(4,5) kernel on grids that fill the chip (OFX_CONV_NO_WINOGRAD or
                                                    OFX_CONV_NO_WINOGRAD15: never); OFX_CONV_TILE_WINOGRAD forces it as above. */
    const float* wino4_w;                        /* optional (3x3 layers): the operand of ofx_wino44_conv_weight.  When set, a
                                                    layer runs the fused Winograd F(4x4,3x3) kernel (2.25 multiplies per output;
                                                    a larger rounding error than F(2x2,3x3)) if all of
                                                    these hold:
                                                    - fp32, stride 1, 'same' padding, a map of whole 16x32 patches;
                                                    - plain epilogue, ReLU or identity, no addend;
                                                    - `res`, a fused norm (`nmean` / `nrstd`, single input segment, at most 1744
                                                      channels) and ofx_conv2d_stats are taken by the kernel's fused variants
                                                      under the rules of `wino_w` above, the partials one row per 16x32 patch
                                                      (plan path 4; a descriptor with none of them: the plain kernel, path 3);
                                                    - the grid fills whole rounds of the chip (at least 768 workgroups of one
                                                      16x32 patch x 64 output channels).
                                                    Otherwise, or with OFX_CONV_NO_WINOGRAD4 (or OFX_CONV_NO_WINOGRAD) in the
                                                    environment, the layer runs as `wino_w` and the rules above decide.
                                                    tile = OFX_CONV_TILE_WINOGRAD4 forces it at any grid size and is rejected
                                                    (OFX_EINVAL) when the layer does not qualify; a forced launch takes two
                                                    segments of whole 16-channel slabs (every other launch: 32).  NULL: as before. */
} ofx_conv_desc;
#define OFX_CONV_TILE_WINOGRAD 1
#define OFX_CONV_TILE_WINOGRAD4 2

int ofx_conv2d(const ofx_conv_desc* d, void* stream);
/* What the launcher would do with `d`, without doing it: the validation and the plan of ofx_conv2d (stats_cap_floats = 0), of
 * ofx_conv2d_stats with room for stats_cap_floats floats, or (want_pool != 0, internal) of the correlation-volume GEMM that also
 * writes pyramid level 1.  Only the numbers of `d` and whether its pointers are set and aligned are looked at: no operand is read
 * and no device is needed.  Returns what the launch would return for an invalid descriptor, and OFX_EINVAL for a GEMM whose
 * output extent is beyond 2 GiB (it runs in row ranges, each with a plan of its own).  In `tile` terms: a direct launch runs the
 * BM x BN tile with chunk length BK that `tile` = BK*1000000 + BM*1000 + BN names, `ks` = 2 being its 2000000000 marker. */
typedef struct ofx_conv_plan {
    int path;                /* 0 direct implicit-GEMM kernel, 1 fused Winograd F(2x2,3x3), 2 fused Winograd F(4,5), 3 fused Winograd
                                F(4x4,3x3), the plain kernel, 4 F(4x4,3x3) with a residual merge, a fused norm or statistics (a
                                descriptor with `res`, `nmean` or under ofx_conv2d_stats never plans to 3); 1 / 2 / 3 / 4: only
                                `stats_rows` below is meaningful (3: always 0) */
    int bm, bn, wm, wn, bk;  /* workgroup tile, wave tile, K chunk */
    int prec;                /* arithmetic of the kernel: OFX_PREC_*, after the split-bf16 modes have mapped the tile onto theirs */
    int ks;                  /* 2: paired K pipelines (64x64 tile on small grids), else 1 */
    int ksplit;              /* > 1: split-K over that many workgroups per tile (needs splitk_ws) */
    int mode;                /* A-side schedule: 0 general gather, 1 scalar chunk coordinates, 2 halo patch */
    int mtiles, ntiles, group_m;   /* grid = mtiles * ntiles * ksplit workgroups per z; group_m: M-tiles per raster group */
    int stats_rows;          /* rows per image ofx_conv2d_stats would report, 0: not produced */
} ofx_conv_plan;
int ofx_conv2d_plan(const ofx_conv_desc* d, size_t stats_cap_floats, int want_pool, ofx_conv_plan* out);
/* host-side helper: OIHW fp32 -> packed [Cout][Kpad] with Cin padded to cin_pad (>= Cin, %4==0).
 * Returns Kpad (or negative error).  `out` may be NULL to query the size. */
long ofx_pack_conv_weight(const float* w_oihw, int Cout, int Cin, int KH, int KW, int cin_pad,
                          float* out);
/* Host-side: packed fp32 weights [n_floats] (n_floats % 4 == 0) -> the pre-split bf16x3 operand format: every
 * group of four consecutive k becomes 16 bytes [hi0 hi1 hi2 hi3 | lo0 lo1 lo2 lo3] with hi = bf16(x),
 * lo = bf16(x - hi), both round-to-nearest-even -- bit-identical to what the kernel's on-the-fly split makes.
 * Same size as the input; use with precision = OFX_PREC_BF16X3_W. Returns 0 or OFX_EINVAL. */
int ofx_split_conv_weight(const float* packed, long n_floats, float* out);
/* Host-side: OIHW fp32 3x3 weights -> the Winograd F(2x2,3x3) operand of ofx_conv_desc.wino_w: U = G g G^T per channel pair,
 * computed in float64 and rounded once, stored [16 points][Cout rounded up to 64][Cin] in the kernel's operand order (the
 * exact index is documented at the definition, conv_wino.hip).  Cin % 16 == 0.  Returns the float count (`out` may be NULL
 * to query it) or OFX_EINVAL. */
long ofx_wino_conv_weight(const float* w_oihw, int Cout, int Cin, float* out);
/* Host-side: OIHW fp32 1x5 or 5x1 weights (KH, KW) -> the 1D Winograd F(4,5) operand of ofx_conv_desc.wino_w: U = G g per
 * channel pair over the points {0, 1, -1, 2, -2, 1/2, -1/2, inf}, computed in float64 and rounded once, stored [8 points][Cout
 * rounded up to 128][Cin] in the kernel's operand order (the exact index is documented at the definition, conv_wino.hip).
 * Cin % 16 == 0.  Returns the float count (`out` may be NULL to query it) or OFX_EINVAL. */
long ofx_wino15_conv_weight(const float* w_oihw, int Cout, int Cin, int KH, int KW, float* out);
/* Host-side: OIHW fp32 3x3 weights -> the Winograd F(4x4,3x3) operand of ofx_conv_desc.wino4_w: U = G g G^T per channel pair
 * over the points {0, 1, -1, 2, -2, inf}, computed in float64 and rounded once, stored [36 points][Cout rounded up to 64][Cin]
 * in the kernel's operand order (the exact index is documented at the definition, conv_wino.hip).  Cin % 16 == 0.  Returns the
 * float count (`out` may be NULL to query it) or OFX_EINVAL. */
long ofx_wino44_conv_weight(const float* w_oihw, int Cout, int Cin, float* out);
/* The same for the three-piece arithmetic (OFX_PREC_BF16X6_W): `out` holds 1.5 * n_floats floats -- first the [hi x4 | mid x4] groups
 * (16 bytes per four consecutive k), then the [lo x4] groups (8 bytes per four k); hi + mid + lo = x exactly unless lo underflows.
 * The whole matrix [Cout][Kpad] must be converted in one call (the lo groups are addressed from its end): a convolution that uses it
 * passes d->Cout = that row count and d->nz <= 1 (a row slice or a batched GEMM would read the lo groups from the wrong place;
 * ofx_conv2d returns OFX_EINVAL for nz > 1, and for a precision outside OFX_PREC_FP32 .. OFX_PREC_F16). */
int ofx_split_conv_weight3(const float* packed, long n_floats, float* out);
/* Host-side: packed fp32 weights [n_floats] -> IEEE halves [n_floats] (2 * n_floats bytes in `out_halves`), the operand of
 * OFX_PREC_F16_W and, for the folded weights of ofx_upconv2x_weight, of ofx_upconv2x_prec with that precision.  Round-to-nearest-even,
 * bit-identical to the kernels' convert: fp16 subnormals are produced (not flushed), a magnitude that rounds beyond 65504 becomes an
 * infinity, NaN stays NaN.  Returns 0, or OFX_EINVAL for a NULL pointer or n_floats <= 0. */
int ofx_half_conv_weight(const float* packed, long n_floats, void* out_halves);

/* instance norm statistics over HW per (b,c): mean and 1/sqrt(var+eps) (biased var), NHWC input with rows of ld >= C floats
 * (ld > C: the statistics of a channel slice).  C % 4 == 0, C <= 256, ld % 4 == 0 and x 16-byte aligned: OFX_EALIGN otherwise.
 * scratch: max(B*64, min(B,7)*256) * C * 2 doubles (f64 partial sums per image slice), 8-byte aligned. */
int ofx_inorm_stats(const float* x, int ld, float* mean, float* rstd, float* scratch,
                    int B, long HW, int C, float eps, void* stream);
/* ofx_conv2d that also leaves per-channel (sum, sum of squares) partials of the outputs it writes in `part`, as
 * [B][*rows_per_image][Cout][2] floats, when the launch can produce them: plain epilogue, identity activation, no `res`, tiles
 * that stay inside one image, and at most part_floats floats.  Every precision of the direct kernels produces them (the sums are
 * fp32 sums of the stored fp32 outputs whatever the arithmetic of the products; the split-bf16 modes map the tile onto 128x128,
 * 128x64 or 64x64 first, so their row count can differ from the fp32 launch of the same layer).  *rows_per_image = 0: not
 * produced (use ofx_inorm_stats).  Both the direct and the fused Winograd kernels write them, in a fixed order (repeats are
 * bit-identical). */
int ofx_conv2d_stats(const ofx_conv_desc* d, float* part, size_t part_floats, int* rows_per_image, void* stream);
/* mean and 1/sqrt(var+eps) (biased var) per (b,c) [B][C] from ofx_conv2d_stats' partials of HW pixels per image (the `rows` rows
 * of an image added in a fixed order) */
int ofx_inorm_finalize(const float* part, float* mean, float* rstd, int B, int rows, long HW, int C, float eps, void* stream);
/* out = relu?( (x-mean)*rstd ) ; with res: out = relu( r + relu((x-mean)*rstd) ) where
 * r = res (res_mean==NULL) or (res-res_mean)*res_rstd -- or relu of that when bit 1 of `relu` is set (relu = 3: the residual is
 * itself the raw output of a normalised + ReLU layer, RAFT/core/extractor.py:160-165 feeding :44-56).  C % 4 == 0 and C <= 1024 (a thread keeps one channel quad:
 * OFX_EINVAL beyond); any B (batches over 65535 images are split into several launches). */
int ofx_inorm_apply(const float* x, const float* mean, const float* rstd, const float* res,
                    const float* res_mean, const float* res_rstd, float* out, int B, long HW, int C,
                    int relu, void* stream);
/* u8 HWC3 image -> f32 NHWC4 (4th channel 0), value 2*(x/255)-1 (raft.py:89-90); bgr=1 swaps to RGB */
int ofx_preprocess_u8(const uint8_t* img, float* out, long npix, int bgr, void* stream);

/* ---------------------------------------------------------------- correlation */
/* vol0[b,i,j] = <f1[b,i,:], f2[b,j,:]> / sqrt(D) and the avg-pooled pyramid (CorrBlock.__init__).
 * f1,f2: [B, h*w, D] (NHWC).  pyr[l] holds, for each of the B*h*w source pixels, that pixel's h_l x w_l slice
 * (h_l = h >> l, floor) in the BLOCKED layout the lookup reads: 4-row x 8-column blocks of 32 floats (128 bytes = one
 * HBM line), blocks row-major, padding elements zero:
 *     slice[((y / 4) * ceil(w_l / 8) + x / 8) * 32 + (y % 4) * 8 + (x % 8)] = corr(pixel, (y, x))
 * so pyr[l] is [B*h*w][ofx_corr_slice_floats(h_l, w_l)] and must be 16-byte aligned.  levels in [1,4]. */
int ofx_corr_slice_floats(int h_l, int w_l);      /* ceil(h_l/4) * ceil(w_l/8) * 32 */
int ofx_corr_volume(const float* f1, const float* f2, float* const* pyr, int B, int h, int w, int D,
                    int levels, void* stream);
/* The same pyramid on the "A-stationary" volume kernel (csrc/corr_split.hip: all of K = 256 for a wave's rows in registers, the other
 * operand streamed through LDS, whole-line stores):
 *   planes = 1 -> exact fp32 on v_mfma_f32_32x32x2_f32: BIT-IDENTICAL to ofx_corr_volume on every level (what ofx_raft_forward runs
 *                 wherever the batch fills the part);
 *   planes = 2 -> "bf16x3" (opt-in; RAFT/core/corr.py:52-60 computes in fp32): each fp32 operand = hi + lo bf16, products hh + hl + lh,
 *                 ~16 mantissa bits;
 *   planes = 3 -> "bf16x6" (opt-in): hi + mid + lo, the six products >= 2^-16: fp32-level accuracy;
 * both split forms on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  shared_f2 != 0: f2 is ONE feature map [h*w, D] shared by the
 * B pairs (a key frame).  Needs D == 256, h % 8 == 0, w % 16 == 0, levels >= 2 and (h*w)^2 * 4 < 2 GiB per pair; anything else returns
 * OFX_EINVAL (use ofx_corr_volume). */
int ofx_corr_volume_split(const float* f1, const float* f2, float* const* pyr, int B, int h, int w, int D,
                          int levels, int planes, int shared_f2, void* stream);
/* CorrBlock.__call__ on the blocked pyramid: out[m, l*(2r+1)^2 + i*(2r+1) + j] for coords [B*h*w][2];
 * out row stride ldo */
int ofx_corr_lookup(const float* const* pyr, const float* coords, float* out, int ldo, int B, int h,
                    int w, int levels, int radius, void* stream);
/* alt_cuda_corr.forward: fmap1 [B,H1,W1,C], fmap2 [B,H2,W2,C], coords [B,N,H1,W1,2] ->
 * corr [B,N,(2r+1)^2,H1,W1] (overwritten, not accumulated into).  C % 4 == 0. */
int ofx_local_corr_fwd(const float* fmap1, const float* fmap2, const float* coords, float* corr,
                       int B, int H1, int W1, int H2, int W2, int C, int N, int r, void* stream);
/* alt_cuda_corr.backward (correlation_kernel.cu:122-256,288-324): gradients of ofx_local_corr_fwd with respect to
 * the two feature maps for corr_grad f32[B,N,(2r+1)^2,H1,W1]; fmap1_grad f32[B,H1,W1,C] and fmap2_grad
 * f32[B,H2,W2,C] are overwritten (the reference returns fresh zero-initialised tensors; its third output,
 * coords_grad, is all zeros and is left to the caller).  fmap2_grad is accumulated with float atomics like the
 * reference's atomicAdd, so its low-order bits depend on scheduling.  Training-only in the reference. */
int ofx_local_corr_bwd(const float* fmap1, const float* fmap2, const float* coords, const float* corr_grad,
                       float* fmap1_grad, float* fmap2_grad, int B, int H1, int W1, int H2, int W2, int C, int N,
                       int r, void* stream);
/* The engine's volume-free lookup (AlternateCorrBlock.__call__, corr.py:74-91, all levels at once): fmap1 [n1,H1,W1,C];
 * fmap2_levels: HOST array of `levels` device pointers, level l = [n2,H1>>l,W1>>l,C] (the 2x2-average-pooled maps, once per unique
 * image); coords [B,H1,W1,2] on the level-0 grid (level l samples at coords / 2^l); idx1 / idx2: DEVICE int arrays, the image of
 * fmap1 / fmap2 pair b uses -- NULL = image b, all zeros = one image shared by the batch.  Writes columns [0, levels * (2r+1)^2) of
 * rows [B*H1*W1][ld] (level-major, then x-major as alt_cuda_corr), scaled by 1/sqrt(C); the other columns are not touched.
 * tiled = 1: the LDS-tiled kernel (csrc/corr_local_tiled.hip; radius 3 or 4, C % 16 == 0, B <= 65535); tiled = 0: one launch of
 * ofx_local_corr_fwd's per-pixel kernel per level (idx1 = idx2 = NULL only, radius <= 4, C % 4 == 0).  Taps outside a map count as
 * zero; a pixel whose scaled coordinate is NaN, infinite or beyond 1e7 in magnitude gets zeros. */
int ofx_local_corr_rows(const float* fmap1, const float* const* fmap2_levels, const int* idx1, const int* idx2,
                        const float* coords, float* rows, int ld, int B, int H1, int W1, int C, int levels, int radius,
                        int tiled, void* stream);
/* 2x2 average pool of an NHWC tensor (AlternateCorrBlock pyramid, corr.py:68-72) */
int ofx_avgpool2_nhwc(const float* in, float* out, int B, int H, int W, int C, void* stream);

/* convex 8x upsample: coords1 [B*h*w][2], mask [B*h*w][576] -> flow_up f32[B, 8h, 8w, 2] */
int ofx_upsample_flow(const float* coords1, const float* mask, float* flow_up, int B, int h, int w,
                      void* stream);
/* ofx_upsample_flow + the bilinear backward warp of one shared frame u8 [8h][8w][3] in ONE kernel (the flow of a lane's four fine
 * pixels is sampled while it is still in registers): warped u8 [B][8h][8w][3]; flow_up f32 [B][8h][8w][2] or NULL (not written).
 * sign = +1 (PDCNet convention, pdcnet_of.py:34-42) or -1 (RAFT convention, ofgen_keyframe_inpaint.py:92-98).
 * Bit-identical to ofx_upsample_flow followed by ofx_warp_u8(OFX_WARP_BILINEAR) with frame_batch_stride = 0. */
int ofx_upsample_flow_warp(const float* coords1, const float* mask, float* flow_up, const uint8_t* frame,
                           uint8_t* warped, int B, int h, int w, float sign, void* stream);
/* upflow8 of the small network (RAFT/core/utils/utils.py:80-82, raft.py:134-135): flow = coords1 - coords0 on the coarse grid,
 * bilinear upsampled with align_corners=True to [8h, 8w] and multiplied by 8 (8 * F.interpolate(flow, (8h, 8w), 'bilinear',
 * align_corners=True)).  coords1 [B*h*w][2] (8-byte aligned) -> flow_up f32[B, 8h, 8w, 2] (16-byte aligned); any h, w >= 1. */
int ofx_upflow8(const float* coords1, float* flow_up, int B, int h, int w, void* stream);
/* ofx_upflow8 + the bilinear backward warp of one shared frame u8 [8h][8w][3] in ONE kernel (the counterpart of
 * ofx_upsample_flow_warp for the small network): warped u8 [B][8h][8w][3]; flow_up f32 [B][8h][8w][2] or NULL (not written).
 * sign = +1 (pdcnet_of.py:34-42) or -1 (ofgen_keyframe_inpaint.py:92-98).
 * Bit-identical to ofx_upflow8 followed by ofx_warp_u8(OFX_WARP_BILINEAR) with frame_batch_stride = 0. */
int ofx_upflow8_warp(const float* coords1, float* flow_up, const uint8_t* frame, uint8_t* warped, int B, int h, int w,
                     float sign, void* stream);
/* The flow head's second convolution (update.py:6-14, 3x3, 256 -> 2) fused with coords1 += delta (raft.py:131), as the RAFT
 * executor runs it.  x [B*h*w][ldx] NHWC fp32, the first 256 channels read (ldx >= 256, ldx % 4 == 0, 16-byte aligned);
 * w [2][kpad] as ofx_pack_conv_weight packs the OIHW [2][256][3][3] weight (kpad >= 2304, kpad % 4 == 0, 16-byte aligned);
 * bias [2]; coords1 [B*h*w][2] (8-byte aligned).  Per pixel m = (b*h + y)*w + x, channel o in {0, 1}:
 *   coords1[m*2 + o] += conv + bias            (delta first, then the add: one rounding at the coordinate's magnitude)
 *   hx_flow[m*ldh + o] = coords1[m*2 + o] - (o == 0 ? x : y)          (ldh >= 2)
 *   frows[m*16 + 2*s + o] = the hx_flow value of pixel x + s - 3 of the same row, for slot s = 0..6, written only where that
 *                           pixel is inside the image (convf1's 7-wide row of flows)
 * Nothing else is written: slots of neighbours outside the image, floats 14 and 15 of every row and the other channels of an hx
 * row keep what they held.  B*h*w*ldx*4 < 2^31 (32-bit byte offsets).  OFX_EINVAL for a null pointer, a non-positive size or a
 * short ldx / kpad / ldh, OFX_EALIGN for the alignments above. */
int ofx_flow_head(const float* x, int ldx, const float* w, int kpad, const float* bias, float* coords1, float* hx_flow,
                  int ldh, float* frows, int B, int h, int w_, void* stream);

/* forward_interpolate of RAFT/core/utils/utils.py:26-53 (the warm start of a video chain, OFX_RAFT_FLOW_INIT): flow f32[B,h,w,2] ->
 * out f32[B,h,w,2] (the flow_low layout; fields independent; out must not be flow).  Every pixel (x0, y0) is a source at
 * (x1, y1) = (x0 + dx, y0 + dy) in float64, valid iff 0 < x1 < w and 0 < y1 < h (strict); every output pixel takes the (dx, dy) of
 * the valid source nearest to its integer position by the float64 squared distance (x1-x0)^2 + (y1-y0)^2 (no FMA) -- scipy's
 * griddata(method='nearest').  Ties: the lowest source index (y0 * w + x0).  A field without a valid source gives NaN everywhere.
 * Exact whatever the field; cost grows with the distance to the nearest source (large holes approach O(h*w) per pixel).
 * scratch: ofx_forward_interpolate_scratch_bytes(B, h, w) bytes, 4-byte aligned (0 = unsupported size: h*w >= 2^30). */
size_t ofx_forward_interpolate_scratch_bytes(int B, int h, int w);
int ofx_forward_interpolate(const float* flow, float* out, void* scratch, size_t scratch_bytes, int B, int h, int w, void* stream);

/* ---------------------------------------------------------------- RAFT engine */
typedef struct ofx_tensor {            /* one entry of a checkpoint state_dict (host memory, fp32) */
    const char* name;                  /* reference key, e.g. "fnet.layer1.0.conv1.weight"        */
    const float* data;
    int ndim; long shape[4];
} ofx_tensor;

typedef struct ofx_raft ofx_raft;      /* opaque */

/* Builds the engine on the current device: packs and uploads all weights (folds cnet BatchNorm into
 * per-channel scale/shift).  Keys may carry the "module." DataParallel prefix. */
int ofx_raft_create(const ofx_tensor* tensors, int n, ofx_raft** out);
int ofx_raft_destroy(ofx_raft* r);
/* bytes of device workspace needed for a batch of B pairs of HxW images (H,W multiples of 8), whatever the flags: the larger of the
 * two correlation layouts (the volume's) */
size_t ofx_raft_workspace_bytes(const ofx_raft* r, int B, int H, int W);
/* bytes of the layout a call with these `flags` actually carves (OFX_RAFT_ALT_CORR: no correlation pyramid; OFX_RAFT_SHARED_IMG1/2:
 * one feature map instead of B; the other flags do not change the layout).  n_images = 0: ofx_raft_forward / _forward_warp;
 * n_images > 0: the indexed-pairs entry points (the shared flags are invalid there).  A forward call succeeds with a workspace of
 * exactly this size.  0 = bad arguments.  r may be NULL (the basic network). */
size_t ofx_raft_workspace_bytes_mode(const ofx_raft* r, int n_images, int B, int H, int W, int flags);

#define OFX_RAFT_BGR          1   /* input images are BGR (calc) instead of RGB (calc_batch)       */
#define OFX_RAFT_SHARED_IMG2  2   /* image2 is ONE image shared by the whole batch (key frame)     */
#define OFX_RAFT_SHARED_IMG1  4   /* image1 is ONE image shared by the whole batch                 */
#define OFX_RAFT_ALT_CORR     8   /* on-the-fly local correlation instead of the volume (alt_cuda_corr): every entry point, both
                                     networks, with the shared-image flags and OFX_RAFT_FLOW_INIT; pooled fmap2 levels exist once per
                                     unique image.  Runs the LDS-tiled kernel (ofx_local_corr_rows); OFX_LOCAL_CORR_NO_TILED=1 in the
                                     environment (read once per process) puts it back on the per-pixel kernel */
#define OFX_RAFT_BF16X3      16   /* opt-in: split-bf16 matrix-core arithmetic for every convolution / the volume */
#define OFX_RAFT_BF16X6      64   /* opt-in: three-piece split-bf16 arithmetic (OFX_PREC_BF16X6) for every convolution / the volume */
#define OFX_RAFT_BN_BATCH   128   /* context-encoder BatchNorm on the statistics of the image itself (the reference's RAFT_2 as written:
                                     a model never put in .eval(), one image per call) instead of the folded running statistics */
#define OFX_RAFT_SEPARATE_STATS 256 /* diagnostic: instance-norm statistics by their own f64 pass over the stored tensor instead of
                                     out of the convolution epilogues (fp32 partial sums per wave) */
#define OFX_RAFT_VOL_BF16X3  512  /* opt-in: ONLY the correlation-volume GEMM in split-bf16 (hi + lo) arithmetic, operands pre-split into
                                     bf16 planes (ofx_corr_volume_split); every convolution stays exact fp32 */
#define OFX_RAFT_VOL_BF16X6 1024  /* the same with three planes per operand (fp32-level accuracy) */
#define OFX_RAFT_SERIAL       32  /* keep every launch on the caller's stream (default: small batches run their
                                     independent chains on internal side streams, joined before returning) */
#define OFX_RAFT_FLOW_INIT  2048  /* warm start (RAFT.forward(flow_init=...), raft.py:118-119): flow_low is in/out and must be non-NULL
                                     (else OFX_EINVAL) and 8-byte aligned.  It is read at the start of the call as the initial flow
                                     f32[B,H/8,W/8,2], one field per pair in pair order (the padded 1/8 grid), and overwritten with the
                                     final low-resolution flow.  coords1 = coords0 + init (one fp32 rounding); the first iteration sees
                                     the flow (coords0 + init) - coords0.  Every entry point and both networks; without the flag nothing
                                     changes.  ofx_forward_interpolate makes the init of the next pair of a video from this one's. */
#define OFX_RAFT_F16 4096         /* opt-in, the basic network only: every convolution of the encoders and the update block in
                                     the fp16 arithmetic (descriptors with OFX_PREC_F16_EPI; the reference's args.mixed_precision, RAFT/core/raft.py:99,110,127).  Rounded to
                                     half: the two operands of each convolution as they are staged, nothing else.  Not rounded: the
                                     activations in memory, the feature maps, the correlation volume (exact fp32 as in the reference,
                                     which casts the maps back with .float(); OFX_RAFT_VOL_BF16X3 / _BF16X6 stay independent and may
                                     be combined), the lookup, the flow head, coords1 + delta and the convex upsample -- a subset of
                                     autocast's roundings.  With OFX_RAFT_BF16X3 or _BF16X6: OFX_EINVAL.  The convolutions get no
                                     split-K workspace in this mode (that arithmetic has no split-K kernels), so small grids run
                                     unsplit: a single pair may be slower than in fp32.  Flow EPE vs float64 ~1e-2 px after 20
                                     iterations (fp32: ~5e-6): the 1e-3 px bar of the default path does not apply */

/* RAFT.forward(test_mode=True): image1/image2 u8 [B,H,W,3] on device -> flow_up f32[B,H,W,2]
 * (flow on image1's grid pointing into image2) and, if non-NULL, flow_low f32[B,H/8,W/8,2].
 * One call takes at most (2^31 - 4096) / ((H/8)*(W/8)*3072) pairs (113 at 512x768): the kernels address their
 * operands with 32-bit byte offsets; OFX_EINVAL beyond that -- pairs are independent, slice the batch. */
int ofx_raft_forward(ofx_raft* r, const uint8_t* image1, const uint8_t* image2, int B, int H, int W,
                     int iters, int flags, float* flow_up, float* flow_low, void* workspace,
                     size_t workspace_bytes, void* stream);
/* The same forward with the backward warp of ONE shared uint8 RGB frame (the rendered AI key frame) done inside the convex
 * upsample -- the tail of the hot path (pdcnet_of.py:34-42 in its bilinear mode; warp_sign = +1: out(y,x) = frame(y + fy, x + fx),
 * -1: the RAFT-side convention of ofgen_keyframe_inpaint.py:92-98): warped u8 [B,H,W,3] = the bilinear warp of warp_frame u8 [H,W,3]
 * along the final flow, bit-identical to ofx_raft_forward followed by ofx_warp_u8(bilinear).  flow_up may be NULL (then the full-
 * resolution flow is never written: 201 MB less traffic per 64 frames at 512x768). */
int ofx_raft_forward_warp(ofx_raft* r, const uint8_t* image1, const uint8_t* image2, int B, int H, int W,
                          int iters, int flags, float* flow_up, float* flow_low, const uint8_t* warp_frame,
                          float warp_sign, uint8_t* warped, void* workspace, size_t workspace_bytes, void* stream);
/* Indexed pairs ("next" row f1, KeyframeConv / calculate_pairwise, ofgen_keyframe_inpaint.py:627-668):
 * n_images unique uint8 frames [n,H,W,3] on the device and B pairs (idx1[b], idx2[b]) given as HOST int
 * arrays; flow b is defined on image idx1[b] and points into image idx2[b].  Every image is encoded once
 * (feature + context network), so N*(N-1) ordered pairs cost N encoder passes instead of 3*N*(N-1). */
size_t ofx_raft_workspace_bytes_pairs(const ofx_raft* r, int n_images, int B, int H, int W);
int ofx_raft_forward_pairs(ofx_raft* r, const uint8_t* images, int n_images, const int* idx1,
                           const int* idx2, int B, int H, int W, int iters, int flags, float* flow_up,
                           float* flow_low, void* workspace, size_t workspace_bytes, void* stream);
/* ofx_raft_forward_pairs with the tail of ofx_raft_forward_warp for its FIRST n_warp pairs: warped u8 [n_warp,H,W,3] = the bilinear
 * backward warp of the shared frame warp_frame u8 [H,W,3] along the final flow of pair b < n_warp, produced inside the convex upsample.
 * This is the call behind pdcnet_of's `calc_batch_device(..., warp_frame=)`: pairs [0, n) = frame -> key frame (warped: pdcnet_of.py:34-42
 * in its bilinear mode), pairs [n, 2n) = key frame -> frame (only feed the forward-backward confidence, no warp). */
int ofx_raft_forward_pairs_warp(ofx_raft* r, const uint8_t* images, int n_images, const int* idx1,
                                const int* idx2, int B, int H, int W, int iters, int flags, float* flow_up,
                                float* flow_low, const uint8_t* warp_frame, float warp_sign, int n_warp,
                                uint8_t* warped, void* workspace, size_t workspace_bytes, void* stream);
/* Which network the checkpoint given to ofx_raft_create holds: 0 = basic (raft-things.pth: BasicEncoder, SepConvGRU, convex
 * upsample), 1 = small (raft-small.pth: SmallEncoder, radius-3 lookup, ConvGRU, upflow8; RAFT/core/raft.py:29-33, :48-51).
 * ofx_raft_create picks it from the key set (update_block.gru.convz + fnet.layer1.0.conv3 = small); a dict with keys of both or a
 * partial one is OFX_EKEY.  The small network takes every entry point and flag above except the split-bf16 modes and fp16
 * (OFX_RAFT_BF16X3, _BF16X6, _VOL_BF16X3, _VOL_BF16X6, _F16: OFX_EINVAL) -- it runs in exact fp32 only; OFX_RAFT_BN_BATCH has no meaning for it (no
 * BatchNorm) and is ignored; its launches always stay on the caller's stream (OFX_RAFT_SERIAL implied).  Its widest convolution
 * operand is the 256-float GRU row, so one call takes up to (2^31 - 4096) / ((H/8)*(W/8)*1024) pairs. */
int ofx_raft_variant(const ofx_raft* r);
/* debug / stage-parity access to the buffers of the last forward: returns a device pointer and
 * element count for a named intermediate ("fmap1","fmap2","hx","corr","pyr0".."pyr3","mask",...).  The small network's
 * (ofx_raft_forward / _warp only): "fmap1", "fmap2" ([n][h*w][128]), "hx" (rows of 256: net 0..95, inp 96..159, motion 160..239,
 * flow 240..241, zeros), "corr" (rows of 224: the 196 lookup features of the last iteration, then zeros), "coords1", "pyr0".."pyr3". */
int ofx_raft_buffer(const ofx_raft* r, const char* name, void** ptr, size_t* nfloats);

#ifdef __cplusplus
}
#endif
#endif /* OFX_H */
