/* adain_hip.h — C ABI of the MI355X (gfx950) AdaIN style-transfer inference path.
 *
 * The reference (Ayushkuruvilla/Applied-Image-Processing) has no FFI: its hot path is plain Python
 * over torch ops (Style_3DGS/AdaIN/{function,net,test}.py).  These entry points are what a binding
 * for that path would call instead of torch; each cites the reference code it replaces.  The
 * Python host side (the modules under applied-image-processing_amd/AdaIN/) binds them with ctypes and keeps the
 * reference's function names, argument meaning and error behaviour.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless named *_host; fp32 everywhere;
 *   - the caller allocates every buffer, including workspaces sized by the *_bytes queries;
 *   - images are NCHW (the reference's tensor layout); activations between the encoder and the
 *     decoder are NHWC ("channels last"): [n][h][w][c];
 *   - `stream` is a hipStream_t (NULL = the default stream); every call only enqueues work;
 *   - return value 0 = ok, negative = error (ADAIN_E*); adain_last_error() gives the text of the
 *     calling thread's last error.  No exceptions cross the ABI.  No call allocates, frees or
 *     synchronises, so every call may be captured into a hipGraph.  (Tested launch by launch: tests/capture_cases.py holds a row
 *     per launch declared here, tests/test_gpu_graph_capture.py captures and replays each; the one exception is adain_tvl1_flow.)
 */
#ifndef ADAIN_HIP_H
#define ADAIN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: adain_encode_u8, adain_u8_to_f32 and adain_stylize_u8* added; the direct / F(2x2,3x3) single-layer entry points removed;
 * adain_conv3x3_wino accepts form 5 only.  Version 1 was never frozen.
 * 3: adain_encode_relu1_1 and the uint8 Pillow-exact resize (adain_resize_pil_bilinear_u8*) added; nothing removed or changed.
 * 4: adain_set_schedule / adain_get_schedule and adain_conv3x3_wino4_split* added; the encoder / decoder / stylize workspaces grow by
 *    the partial-sum slabs of the latency schedule (at most 8 MB; callers that size them with the *_bytes queries need no change). */
#define ADAIN_ABI_VERSION 4
#define ADAIN_OK 0
#define ADAIN_EINVAL (-1)  /* bad argument / unsupported shape */
#define ADAIN_ELAUNCH (-2) /* HIP reported a launch error */

#define ADAIN_SRC_DIRECT 0 /* conv input = source tensor */
#define ADAIN_SRC_UP2X 1   /* conv input = nearest 2x upsample of the source (net.py:10,23,30) */
#define ADAIN_SRC_POOL2 2  /* conv input = MaxPool2d(2,2,ceil_mode=True) of the source (net.py:46,53,66) */

typedef void* adain_stream_t; /* hipStream_t */

/* The shared library is built with -fvisibility=hidden: these entry points are all it exports. */
#ifndef ADAIN_API
#define ADAIN_API __attribute__((visibility("default")))
#endif

ADAIN_API int adain_abi_version(void);
ADAIN_API const char* adain_last_error(void);

/* ---- launch schedule of the CALLING THREAD (enqueue-time state, like the error text; not captured by, and harmless to, hipGraphs) ----
 * The reference's callers work at two operating points: loops that style ONE small frame per call (video/utils.py:261-270,341-350:
 * adain_inference(content_size=256) per video frame; test.py:160: content_size 512 by default) and batch jobs.
 *   ADAIN_SCHEDULE_BATCH (default): every generic 3x3 layer accumulates its input channels in one chain.  A frame's result does not
 *     depend on the batch it is in: single-frame calls, sub-batches of any size and any sharding over GPUs give the same bits.
 *   ADAIN_SCHEDULE_LATENCY: a layer whose launch has fewer tiles than the device has compute units (relu4-level layers of a single
 *     256-class frame: 64-128 tiles for 256 compute units, each walking 256-512 input channels alone) is split along cin over
 *     2-8 workgroups per tile; their output-transformed partial sums are added in a FIXED order by a second kernel (no atomics:
 *     the same call gives the same bits every time).  Results differ from the batch schedule's in the last bits (shorter
 *     accumulation chains: slightly closer to the exact sum) and, unlike it, depend on the launch's batch size.
 * adain_set_schedule returns the previous value (>= 0) or ADAIN_EINVAL. */
#define ADAIN_SCHEDULE_BATCH 0
#define ADAIN_SCHEDULE_LATENCY 1
ADAIN_API int adain_set_schedule(int schedule);
ADAIN_API int adain_get_schedule(void);

/* ---- weights: pack a reference state_dict once (net.vgg / net.decoder, net.py:6-92) ----------------
 * w[i] / b[i] are the OIHW weight and bias tensors of the i-th conv in module order
 * (encoder: state_dict keys 0,2,5,9,12,16,19,22,25,29 ; decoder: 1,5,8,11,14,18,21,25,28).
 * `packed` receives MFMA-fragment-ordered weights + biases; its size is the *_floats query.  A pack writes every float of it (the
 * padding between its 256-byte aligned blocks included): the buffer needs no preparation by the caller. */
ADAIN_API size_t adain_encoder_packed_floats(void);
ADAIN_API size_t adain_decoder_packed_floats(void);
ADAIN_API int adain_encoder_pack(const float* const* w_host_array_of_dev_ptrs, const float* const* b_host_array_of_dev_ptrs,
                       float* packed, adain_stream_t stream);
ADAIN_API int adain_decoder_pack(const float* const* w_host_array_of_dev_ptrs, const float* const* b_host_array_of_dev_ptrs,
                       float* packed, adain_stream_t stream);

/* ---- encoder: vgg[:31](x), conv0 .. relu4_1 (net.py:38-69; test.py:57,63,76-77,185) -----------------
 * image NCHW [n][3][h][w] -> feat NHWC [n][hc][wc][512], hc = ceil(ceil(ceil(h/2)/2)/2) (same for w).
 * layer_events: optional host array of 11 hipEvent_t recorded before layer 0 and after each of the
 * 10 conv launches (profiling only; NULL in production).
 * adain_encode_workspace_bytes answers for the device that is current on the calling thread (its compute-unit count sizes the
 * cin-split slabs of ADAIN_SCHEDULE_LATENCY): ask it with the device current on which the call will run. */
ADAIN_API void adain_encoded_size(int h, int w, int* hc, int* wc);
ADAIN_API size_t adain_encode_workspace_bytes(int n, int h, int w);
ADAIN_API int adain_encode(const float* image_nchw, float* feat_nhwc, const float* packed, void* workspace,
                 size_t workspace_bytes, int n, int h, int w, void* const* layer_events, adain_stream_t stream);

/* adain_encode on a decoded frame as the reference holds it before ToTensor (test.py:16-24, :190-204): image HWC uint8
 * [n][h][w][3].  The first layer's kernel applies ToTensor itself (float(v) / 255, correctly rounded), so the features are
 * bit-identical to adain_encode(ToTensor(image)) while the frame crosses PCIe and HBM as 3 bytes per pixel instead of 12. */
ADAIN_API int adain_encode_u8(const uint8_t* image_nhwc_u8, float* feat_nhwc, const float* packed, void* workspace,
                    size_t workspace_bytes, int n, int h, int w, void* const* layer_events, adain_stream_t stream);

/* The encoder's FIRST fused layer alone: vgg[:4] = conv0 (1x1, the checkpoint's Caffe-style preprocessing: x255, channel swap,
 * mean subtraction) -> ReflectionPad -> conv1_1 -> ReLU (net.py:39-42), which this library computes as ONE layer with conv0 folded
 * into conv1_1's weights and bias.  image: NCHW float [n][3][h][w], or (is_u8) HWC uint8 [n][h][w][3] with ToTensor inside;
 * relu1_1: NHWC [n][h][w][64].  For parity checks of the fold at trained-checkpoint magnitudes (tests/golden/case_g.npz) and as
 * the first of the four taps AdaIN's own loss uses (net.py:110-117, enc_1); adain_encode* run the same kernel as their first launch. */
ADAIN_API int adain_encode_relu1_1(const void* image, int is_u8, float* relu1_1_nhwc, const float* packed, int n, int h, int w,
                         adain_stream_t stream);

/* The same encoder over `count` (1..4) image batches of different sizes in ONE pass: the content batch and the style image
 * of a style_transfer call go through the same vgg (test.py:57,63 / :76-77).  Results are bit-identical to one adain_encode
 * per batch; every generic 3x3 layer is a single launch whose tile list covers all batches, so the small style-branch layers
 * ride in the content launches instead of under-filling the chip on their own.  images[i] NCHW [n[i]][3][h[i]][w[i]] ->
 * feats[i] NHWC.  The pointer arrays and n / h / w are HOST arrays.  layer_events as for adain_encode.
 * adain_encode_multi_workspace_bytes, like adain_encode_workspace_bytes, answers for the device current on the calling thread. */
ADAIN_API size_t adain_encode_multi_workspace_bytes(int count, const int* n, const int* h, const int* w);
ADAIN_API int adain_encode_multi(int count, const float* const* images_nchw, float* const* feats_nhwc, const int* n, const int* h,
                       const int* w, const float* packed, void* workspace, size_t workspace_bytes,
                       void* const* layer_events, adain_stream_t stream);

/* ---- decoder: net.decoder(feat) (net.py:6-36; test.py:71,81) ----------------------------------------
 * feat NHWC [n][hc][wc][512] -> image NCHW [n][3][8hc][8wc].  layer_events: 10 events (before + 9 convs).
 * adain_decode_workspace_bytes, like adain_encode_workspace_bytes, answers for the device current on the calling thread. */
ADAIN_API size_t adain_decode_workspace_bytes(int n, int hc, int wc);
ADAIN_API int adain_decode(const float* feat_nhwc, float* image_nchw, const float* packed, void* workspace,
                 size_t workspace_bytes, int n, int hc, int wc, void* const* layer_events, adain_stream_t stream);

/* ---- calc_mean_std (function.py:4-12): per (n, c) mean and sqrt(unbiased var + eps) over h*w ---------
 * nhwc != 0: feat is [n][hw][c]; nhwc == 0: feat is [n][c][hw].  mean/std: [n][c]. */
ADAIN_API size_t adain_mean_std_workspace_bytes(int nhwc, int n, int c, int hw);
ADAIN_API int adain_mean_std(const float* feat, int nhwc, int n, int c, int hw, float eps, float* mean, float* std_out,
                   void* workspace, size_t workspace_bytes, adain_stream_t stream);

/* ---- adaptive_instance_normalization + blend (function.py:15-23; test.py:69-70, 79-80) -----------------
 * t = (x - c_mean)/c_std * s_std + s_mean ;
 *   alpha form: out = t*alpha + x*one_minus_alpha          (style_transfer_simple; plain AdaIN = 1, 0)
 *   pmap  form: out = t*(1 - P) + x*P, P [pmap_n][hw]      (style_transfer, depth-aware)
 * style_n and pmap_n are 1 (broadcast over the batch) or n. */
ADAIN_API int adain_blend_alpha(const float* content_feat, int nhwc, int n, int c, int hw, const float* c_mean,
                      const float* c_std, const float* s_mean, const float* s_std, int style_n, float alpha,
                      float one_minus_alpha, float* out, adain_stream_t stream);
ADAIN_API int adain_blend_pmap(const float* content_feat, int nhwc, int n, int c, int hw, const float* c_mean,
                     const float* c_std, const float* s_mean, const float* s_std, int style_n, const float* pmap,
                     int pmap_n, float* out, adain_stream_t stream);

/* ---- style interpolation: the blend of a weighted mix of K styles (Style_3DGS/AdaIN/test_video.py:30-45, style_transfer(...,
 * interpolation_weights); its CLI flag --style_interpolation_weights, :77-79) ---------------------------------------------------
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.)
 * One rounding per operation, in the reference's order, no fused multiply-add:
 *   nrm  = (x - c_mean) / c_std                                  function.py:21-22, the same for every style
 *   b_k  = nrm * s_std[k] + s_mean[k]                            function.py:23
 *   feat = w_0 * b_0 ; feat = feat + w_k * b_k, k = 1 .. K-1     test_video.py:37-40 (its 0 + w_0 * b_0 is w_0 * b_0)
 *   alpha form: out = feat*alpha + x*one_minus_alpha             test_video.py:44
 *   pmap  form: out = feat*(1 - P) + x*P, P [pmap_n][hw]         the substitution style_transfer makes for one style (test.py:70)
 * s_mean / s_std [k][c]: ONE set of k styles for the batch, 1 <= k <= ADAIN_MIX_MAX_STYLES.  weights: a DEVICE array
 * [weights_n][k][weights_hw]; weights_n = 1 (one row for every frame) or n (a row per frame: a cross-fade through a clip);
 * weights_hw = 1 (a scalar per style) or hw (a map per style at feature resolution, W[k][pixel] standing where w_k stood).  The
 * weights are used as given: nothing normalises them.  pmap NULL = alpha form; pmap_n 1 or n.  Layout and alignment rules are those
 * of adain_blend_*: c % 4 == 0 for NHWC, n*c*hw % 4 == 0 for NCHW, fewer than 2^31 elements.  Everything else is refused with
 * ADAIN_EINVAL before anything is launched.  With k = 1 and the scalar weight 1.0f the result is adain_blend_alpha's / _pmap's bit
 * for bit (1 * b is exact).  8 bytes of HBM traffic per element whatever k is. */
#define ADAIN_MIX_MAX_STYLES 16
ADAIN_API int adain_blend_mix(const float* content_feat, int nhwc, int n, int c, int hw, const float* c_mean, const float* c_std,
                    const float* s_mean, const float* s_std, int k, const float* weights, int weights_n, int weights_hw,
                    float alpha, float one_minus_alpha, const float* pmap, int pmap_n, float* out, adain_stream_t stream);

/* ---- compute_stylization_strength_map (test.py:119-150) ------------------------------------------------
 * depth [h0][w0] -> pmap [hc][wc]: bicubic resize, min-max normalise, minus mean, sigmoid(prominence*P),
 * clamp(max = 1 - offset); an exactly constant resized map gives zeros (test.py:141-143). */
ADAIN_API size_t adain_strength_map_workspace_bytes(int hc, int wc);
ADAIN_API int adain_strength_map(const float* depth, int h0, int w0, int hc, int wc, float offset, float prominence,
                       float* pmap, void* workspace, size_t workspace_bytes, adain_stream_t stream);

/* ---- content-mask composite of adain_inference (test.py:222-236) ---------------------------------------
 * resize_*: `planes` independent [hi][wi] planes -> [ho][wo]; bilinear = F.interpolate(mode="bilinear",
 * align_corners=False), nearest = F.interpolate(mode="nearest").
 * mask_composite: out = content*(1-m) + stylized*m on NCHW [n][c][hw]; mask [mask_n][mask_c][hw],
 * mask_c in {1, c}, mask_n in {1, n}. */
ADAIN_API int adain_resize_bilinear(const float* in, float* out, int planes, int hi, int wi, int ho, int wo,
                          adain_stream_t stream);
ADAIN_API int adain_resize_nearest(const float* in, float* out, int planes, int hi, int wi, int ho, int wo,
                         adain_stream_t stream);
ADAIN_API int adain_mask_composite(const float* content, const float* stylized, const float* mask, int mask_c, int mask_n,
                         float* out, int n, int c, int hw, adain_stream_t stream);

/* ---- torchvision save_image quantiser (test.py:243-244): NCHW float -> NHWC u8, x*255+0.5 clamped ------ */
ADAIN_API int adain_quantize_u8(const float* image_nchw, uint8_t* out_nhwc, int n, int c, int h, int w,
                      adain_stream_t stream);

/* ---- torchvision ToTensor (test.py:22): NHWC u8 [n][h][w][c] -> NCHW float [n][c][h][w], float(v) / 255 correctly rounded
 * (bit for bit `tensor.float() / 255`); what the mask composite needs of a frame that was uploaded as uint8 ------------------ */
ADAIN_API int adain_u8_to_f32(const uint8_t* in_nhwc, float* out_nchw, int n, int c, int h, int w, adain_stream_t stream);

/* ---- video post-pass (reference video/utils.py:89-105 warp_image + :223-229 blend_images) -------------------
 * HWC uint8 frames [h][w][c]; flow [2][h][w] (x then y displacement, as estimate_optical_flow returns it,
 * video/utils.py:75-86).  out = u8(clip((alpha*cur/255 + one_minus_alpha*warp(prev)/255)*255, 0, 255)), warp =
 * cv2.remap(INTER_LINEAR, BORDER_REFLECT) in OpenCV's uint8 fixed point (map rounded to 1/32 px, 2^15-scaled weights,
 * (sum + 2^14) >> 15).  The flow can come from adain_farneback_flow below (the reference's Farneback estimator on the device) or
 * from the caller. */
ADAIN_API int adain_warp_blend_u8(const uint8_t* cur_u8, const uint8_t* prev_u8, const float* flow, uint8_t* out_u8, int h, int w,
                        int c, float alpha, float one_minus_alpha, adain_stream_t stream);

/* cv2.resize(frames_u8, (wo, ho), interpolation=cv2.INTER_AREA) of the same post-pass (reference video/utils.py:352-353) on
 * n HWC uint8 frames [n][hi][wi][c] -> [n][ho][wo][c].  The true-area branch of OpenCV's resize (both axes shrink or keep
 * their size): equal sizes copy; integer scales box-average in int with round-half-even ((a+b+c+d+2)>>2 for 2x2); other
 * scales use resizeArea_'s float tap tables in OpenCV's accumulation order.  With an axis enlarged OpenCV leaves that branch
 * and so does this call: the 11-bit fixed-point linear pass with "area mode" coefficients (an integer enlargement replicates
 * pixels). */
ADAIN_API int adain_resize_area_u8(const uint8_t* in_u8, uint8_t* out_u8, int n, int hi, int wi, int c, int ho, int wo,
                         adain_stream_t stream);

/* ---- dense optical flow: cv2.calcOpticalFlowFarneback(prev, next, None, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma,
 * 0) of OpenCV 4.x's CPU implementation (reference video/utils.py:75-86 runs it with 0.5, 5, 15, 3, 7, 1.5, 0) --------------------
 * The rules (level schedule, Gaussian level images, polynomial expansion, matrix update, box-blur flow update, flow upscale) are
 * restated at the top of csrc/flow.hip and in NumPy in tests/farneback_ref.py; parity with cv2 itself is not pinned.
 *
 * adain_flow_gray_u8: the callers' frame preparation, n packed RGB frames [n][hi][wi][3] (PIL's channel order) -> gray [n][ho][wo]:
 *   cv2.resize(frame, (wo, ho)) on the BGR frame cv2.imread gives (uint8 INTER_LINEAR: 2048-scaled taps, VResizeLinear's fixed-point
 *   combine; an exact 2x shrink is INTER_AREA's (a+b+c+d+2)>>2, an equal size a copy), then cv2.COLOR_RGB2GRAY applied to that BGR
 *   data: gray = (4899 B + 9617 G + 1868 R + 8192) >> 14.
 * adain_farneback_levels (host only): the pyramid schedule of an h x w frame: *out_levels = the effective `levels` L (L + 1 pyramid
 *   levels); sizes_wh[2k], [2k+1] = width, height of level k (k = 0: full size ... L: coarsest), ksizes[k] / sigmas[k] = its Gaussian.
 *   Each output may be NULL; the arrays need room for levels + 1 entries (pairs) of the REQUESTED levels.
 * adain_farneback_expand: a frame's pyramid (gray uint8 [h][w] -> `pyramid`, adain_farneback_pyramid_bytes): per level k the level
 *   image [h_k][w_k] then its polynomial expansion R [h_k][w_k][5] (OpenCV's channel order y, x, yy, xx, xy), each float block
 *   256-byte aligned, levels in order k = 0, 1, ...  The padding behind a block (up to its 256-byte boundary, counted in
 *   adain_farneback_pyramid_bytes) is not part of the result: no call writes or reads it.  It depends on the frame only: a clip of N frames needs N expansions, each
 *   used as `next` of one pair and `prev` of the following one.
 * adain_farneback_flow: the flow from pyr_prev's frame to pyr_next's (both expanded with the same h, w, pyr_scale, levels) ->
 *   flow_out [2][h][w] (x then y displacement, the layout adain_warp_blend_u8 consumes).
 * One workspace (adain_farneback_workspace_bytes) serves both calls; calls that share it must be ordered (one stream).
 * Refused with ADAIN_EINVAL: flags != 0 (OPTFLOW_USE_INITIAL_FLOW and OPTFLOW_FARNEBACK_GAUSSIAN are not built), pyr_scale outside
 * (0, 1), poly_n not 5 or 7, winsize outside [2, 63], iterations < 1, levels < 0. */
ADAIN_API int adain_flow_gray_u8(const uint8_t* rgb_u8, int n, int hi, int wi, uint8_t* gray_u8, int ho, int wo, adain_stream_t stream);
ADAIN_API int adain_farneback_levels(int h, int w, double pyr_scale, int levels, int* out_levels, int* sizes_wh, int* ksizes, double* sigmas);
ADAIN_API size_t adain_farneback_pyramid_bytes(int h, int w, double pyr_scale, int levels);
ADAIN_API size_t adain_farneback_workspace_bytes(int h, int w);
ADAIN_API int adain_farneback_expand(const uint8_t* gray_u8, int h, int w, double pyr_scale, int levels, int poly_n, double poly_sigma,
                                     float* pyramid, void* workspace, size_t workspace_bytes, adain_stream_t stream);
ADAIN_API int adain_farneback_flow(const float* pyr_prev, const float* pyr_next, int h, int w, double pyr_scale, int levels, int winsize,
                                   int iterations, int flags, float* flow_out, void* workspace, size_t workspace_bytes, adain_stream_t stream);

/* ---- dense optical flow: cv2.optflow.DualTVL1OpticalFlow_create(...).calc(I0, I1, None) of OpenCV 4.x's contrib CPU implementation
 * (reference video/utils.py:75-86 runs it with the defaults below; its driver picks it, :416) ------------------------------------------
 * The rules (scales, centred gradient, cubic remap, thresholding, dual updates, median, stop rule) are restated at the top of
 * csrc/tvl1.hip and in NumPy in tests/tvl1_ref.py; parity with cv2 itself is not pinned.  The fields keep create()'s names; its
 * defaults: tau 0.25, lambda 0.15, theta 0.3, nscales 5, warps 5, epsilon 0.01, innerIterations 30, outerIterations 10, scaleStep 0.8,
 * gamma 0, medianFiltering 5, useInitialFlow 0.
 *
 * adain_tvl1_scales (host only): the effective scale count (*out_nscales) and sizes_wh[2s], [2s+1] = width, height of scale s (s = 0:
 *   full size); sizes_wh needs room for params->nscales pairs.  Either output may be NULL.
 * adain_tvl1_frame_bytes: the size of one prepared frame (per scale, float4 (I, I_x, I_y, 0) per pixel, 256-byte aligned blocks; the
 *   padding behind a block is counted in the size and is not part of the result: no call writes or reads it).
 * adain_tvl1_prepare: n gray frames [n][h][w] -> n prepared frames, frame_bytes apart.  A frame's preparation depends on the frame
 *   only: a clip prepares each frame once and uses it as I1 of one pair and I0 of the next.
 * adain_tvl1_flow: npairs flows at once.  prev_frames / next_frames are DEVICE arrays of npairs pointers to prepared frames (I0 and
 *   I1 of each pair, all prepared with the same h, w and params; one frame may appear in several pairs); flows_out [npairs][2][h][w] (x then y, the layout adain_warp_blend_u8 consumes);
 *   iters_out, if not NULL, a device int array [npairs][nscales][warps] (effective nscales, scale 0 = full size) that receives the
 *   number of inner steps each (scale, warp) executed.  A pair's result does not depend on the batch it runs in.  The frames and
 *   flows_out must be 16-byte aligned (adain_tvl1_prepare's frames at 256-byte aligned addresses are).  Unlike every other call of
 *   this header, adain_tvl1_flow makes the host wait on `stream`: after every outer pass but the last of each warp it copies back how
 *   many pairs have met the stop rule, waits for that copy (hipStreamSynchronize), and skips the remaining launches of the warp when
 *   all have.  So it cannot be captured into a hipGraph.  It returns with the launches after the last such wait (at least the last
 *   outer pass of the finest scale's last warp and the store of the flows) still enqueued: order readers of flows_out / iters_out
 *   on `stream` as for any other call.
 * The workspace (adain_tvl1_workspace_bytes) serves one call at a time.  Refused with ADAIN_EINVAL before anything is launched: gamma != 0,
 * useInitialFlow != 0, medianFiltering other than <= 1 (off), 3 or 5, nscales < 1, negative warps / iterations, scaleStep outside (0, 1],
 * frames smaller than 3 x 3, more than 64 scales.  The size queries return 0 for refused parameters. */
typedef struct adain_tvl1_params {
    double tau, lambda, theta;
    int nscales, warps;
    double epsilon;
    int innerIterations, outerIterations;
    double scaleStep, gamma;
    int medianFiltering, useInitialFlow;
} adain_tvl1_params;
ADAIN_API int adain_tvl1_scales(int h, int w, const adain_tvl1_params* params, int* out_nscales, int* sizes_wh);
ADAIN_API size_t adain_tvl1_frame_bytes(int h, int w, const adain_tvl1_params* params);
ADAIN_API int adain_tvl1_prepare(const uint8_t* gray_u8, int n, int h, int w, const adain_tvl1_params* params, float* prepared,
                                 adain_stream_t stream);
ADAIN_API size_t adain_tvl1_workspace_bytes(int h, int w, int npairs, const adain_tvl1_params* params);
ADAIN_API int adain_tvl1_flow(const float* const* prev_frames, const float* const* next_frames, int npairs, int h, int w,
                              const adain_tvl1_params* params, float* flows_out, int* iters_out, void* workspace, size_t workspace_bytes,
                              adain_stream_t stream);

/* ---- the localized pipeline's foreground colour transfer (Style_3DGS/localized_style_transfer.py:128-168) and the composite around it
 * (:232-238), which the reference computes in numpy on the host --------------------------------------------------------------------------
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.)
 * fg, bg, out: uint8 HWC [h][w][3] of one size.  A region is the set of pixels whose channels do not sum to zero.  Both regions go
 * to Reinhard's l-alpha-beta space, each is projected on its first principal axis (scikit-learn's PCA(n_components=1), >= 1.5 sign
 * rule), the foreground projections are CDF-matched to the background's (np.sort, np.linspace, np.interp restated: csrc/colour.hip
 * lists the rules) and mapped back through the foreground's axis; pixels outside the foreground region are copied.  float64
 * throughout, partial sums in a fixed order: the same inputs give the same bytes on every run, stream and device size.
 * adain_localized_combine_u8: the same with foreground = content * (1 - m) and background = stylised * m built on the fly from the
 *   {0,1} background mask [h][w] (bytes other than 0 and 1 are the caller's to refuse), and out = adjusted * (1 - m) + background.
 * The workspace (adain_colour_transfer_workspace_bytes; 0 for a refused size or when the process has no device to size the sort
 * for; at least 8-byte aligned; both calls take the same) is
 * not passed with a size: it must hold what the query returns.  It starts with an adain_colour_record that the call fills on the
 * device and that stays valid until the workspace is used again.  The calls enqueue 5 kernels and two rocprim radix sorts, allocate
 * nothing, copy nothing to the host and do not wait for the stream - so they CANNOT know the region sizes: an empty region (the
 * reference returns a copy of the foreground, :141-147) or a region of ONE pixel (the reference divides by zero there; no NaNs
 * are reproduced) leaves `out` a copy of the foreground (combine: the plain composite) and says so in `status`; a caller that wants
 * an error for it reads the record after the stream has got there. */
#define ADAIN_COLOUR_FG_EMPTY 1  /* status bits */
#define ADAIN_COLOUR_BG_EMPTY 2
#define ADAIN_COLOUR_FG_SINGLE 4 /* a region of exactly one pixel: no covariance */
#define ADAIN_COLOUR_BG_SINGLE 8
typedef struct adain_colour_region {
    int64_t n;                 /* pixels in the region */
    double mean[3];            /* PCA.mean_ (l, alpha, beta) */
    double component[3];       /* PCA.components_[0]; zeros when n < 2 */
    double explained_variance; /* PCA.explained_variance_[0] */
} adain_colour_region;
typedef struct adain_colour_record {
    adain_colour_region fg, bg;
    int32_t status; /* 0: the transfer ran; otherwise ADAIN_COLOUR_* bits and `out` holds no transfer */
    int32_t reserved;
} adain_colour_record;
ADAIN_API size_t adain_colour_transfer_workspace_bytes(int h, int w);
ADAIN_API int adain_colour_transfer_u8(const uint8_t* fg_u8, const uint8_t* bg_u8, uint8_t* out_u8, int h, int w, void* workspace,
                                       adain_stream_t stream);
ADAIN_API int adain_localized_combine_u8(const uint8_t* content_u8, const uint8_t* stylised_u8, const uint8_t* mask_u8, uint8_t* out_u8, int h,
                                         int w, void* workspace, adain_stream_t stream);

/* ---- colour-preserving stylisation: coral(style, content) (Style_3DGS/AdaIN/function.py:26-67), which adain_inference applies to
 * the transformed style image when preserve_color is set (test.py:201-202) and the reference computes on CPU tensors -------------------
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.)
 * n content images and style_n (1: one style for all, or n: one per content) style images; pair i is (style i or 0, content i).  Each
 * side is either uint8 HWC [k][h][w][3] (x_is_u8 != 0: what adain_resize_pil_bilinear_u8 writes) or float NCHW [k][3][h][w]; the
 * two sides' sizes are independent.  out: float NCHW [n][3][hs][ws], the style images recoloured to their contents' channel
 * statistics, ready for adain_encode; NOT clamped (the reference does not clamp).
 * Per pair: the channel means, unbiased deviations and C = norm norm^T + I of both sides, the symmetric square roots of both C from a
 * Jacobi eigen-solve in float64 (C = (HW - 1) x correlation matrix + I: every eigenvalue is >= 1, so the inverse square root is
 * bounded by 1), folded into one affine map y = A x + b applied to every style pixel in float64 and rounded once to float.  uint8
 * sides are summed as 64-bit integers of the byte values (exact); float sides in float64 over a partition fixed by the image size:
 * the same inputs give the same bytes on every run, stream, batch position and device size.  A uint8 pixel is read as float(v) / 255
 * correctly rounded, as adain_u8_to_f32 and adain_encode_u8 read it.
 * The workspace (adain_coral_workspace_bytes; 0 for a refused shape; 8-byte aligned) starts with n adain_coral_record, one per pair,
 * which the call fills on the device and which stay valid until the workspace is used again.
 * DEGENERATE INPUT: a side with fewer than two pixels, or with a channel whose variance is zero, makes the reference divide by zero
 * and return NaNs.  No NaNs are reproduced: the pair's record gets the matching ADAIN_CORAL_* status bit(s), A = I, b = 0, and the
 * pair's output is a plain copy of its style image (as float); the other pairs of the call are not affected.
 * Refused with ADAIN_EINVAL before anything is launched: style_n other than 1 and n, n outside 1..65535, an image of no pixels or of
 * 2^30 or more, a workspace below the query's or not 8-byte aligned, float images / out not 4-byte aligned.  4 or 5 kernel launches,
 * no allocation, no synchronisation. */
#define ADAIN_CORAL_STYLE_FLAT 1     /* status bits: a channel of the style has zero variance */
#define ADAIN_CORAL_CONTENT_FLAT 2
#define ADAIN_CORAL_STYLE_SINGLE 4   /* the style has a single pixel: no deviation */
#define ADAIN_CORAL_CONTENT_SINGLE 8
typedef struct adain_coral_side {
    int64_t n;       /* pixels */
    int64_t sum[3];  /* uint8 side: the exact sums of the byte values per channel; float side: 0 */
    int64_t sum2[6]; /* uint8 side: the exact sums of byte products rr, rg, rb, gg, gb, bb; float side: 0 */
    double mean[3];  /* per channel, of v / 255 (uint8) or of the float values */
    double std[3];   /* unbiased (HW - 1); 0 where the status says there is none */
} adain_coral_side;
typedef struct adain_coral_record {
    double A[9]; /* row major: out[i] = sum_j A[3 i + j] style[j] + b[i] */
    double b[3];
    adain_coral_side style, content;
    int32_t status; /* 0: the transfer ran; otherwise ADAIN_CORAL_* bits and the output is a copy of the style */
    int32_t reserved;
} adain_coral_record;
ADAIN_API size_t adain_coral_workspace_bytes(int n, int style_n, int hs, int ws, int hc, int wc);
ADAIN_API int adain_coral(const void* style, int style_is_u8, int style_n, int hs, int ws, const void* content, int content_is_u8, int n,
                          int hc, int wc, float* out_nchw, void* workspace, size_t workspace_bytes, adain_stream_t stream);

/* ---- test_transform's Resize [+ CenterCrop] on the device (test.py:16-24, applied at :190-204; video/utils.py:341-350) --------
 * PIL.Image.resize((wo, ho), BILINEAR) of uint8 RGB images, bit for bit (Pillow's ImagingResample: separable triangle filter whose
 * support grows with the shrink factor, double-precision taps converted to 22-bit fixed point, a horizontal pass into a uint8
 * intermediate, then a vertical pass, clip8) - what torchvision's Resize(size) runs on a PIL image.  in: [n][hi][wi][pixel_bytes]
 * with pixel_bytes = 3 (packed RGB) or 4 (Pillow's RGBX storage, 4th byte ignored); out: packed RGB [n][crop_h][crop_w][3] = the
 * window (crop_y0, crop_x0, crop_h, crop_w) of the ho x wo result (CenterCrop(size): top = round((ho - size) / 2), left likewise;
 * no crop: 0, 0, ho, wo).  The result feeds adain_encode_u8 / adain_stylize_u8 directly.  Workspace: the tap tables of both axes. */
ADAIN_API size_t adain_resize_pil_bilinear_u8_workspace_bytes(int hi, int wi, int ho, int wo);
ADAIN_API int adain_resize_pil_bilinear_u8(const uint8_t* in_u8, int pixel_bytes, int n, int hi, int wi, uint8_t* out_rgb_u8, int ho, int wo,
                                 int crop_y0, int crop_x0, int crop_h, int crop_w, void* workspace, size_t workspace_bytes,
                                 adain_stream_t stream);

/* ---- PIL.Image.resize for all six filters (the palette page's _downsample_image, gui/second_page.py; the NEAREST resize of the
 * localized composite; the LANCZOS / BICUBIC resizes of the loaders) -----------------------------------------------------------------
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.)
 * PIL.Image.Image.resize((wo, ho), resample) of uint8 L and RGB images, bit for bit, without box= and without reducing_gap.
 * `filter` is Pillow's integer code: 0 NEAREST, 1 LANCZOS, 2 BILINEAR, 3 BICUBIC, 4 BOX, 5 HAMMING.
 *
 * The five convolution filters (libImaging/Resample.c) share one tap rule, all in double:
 *     BOX      support 0.5  f(x) = 1 for -0.5 < x <= 0.5, else 0
 *     BILINEAR support 1    f(x) = 1 - |x| for |x| < 1, else 0
 *     HAMMING  support 1    x = |x|; 1 at 0; 0 for x >= 1; else with x *= M_PI: sin(x) / x * (0.54f + 0.46f * cos(x)) - the two constants
 *                           are floats widened to double, as Resample.c writes them
 *     BICUBIC  support 2    a = -0.5, x = |x|; ((a + 2) x - (a + 3)) x x + 1 for x < 1; (((x - 5) x + 8) x - 4) a for x < 2; else 0
 *     LANCZOS  support 3    sinc(x) sinc(x / 3) for -3 <= x < 3, else 0; sinc(0) = 1, else x *= M_PI, sin(x) / x
 *   scale = in / out, filterscale = max(scale, 1), support = filter support * filterscale, ksize = (int)ceil(support) * 2 + 1; per
 *   output index xx: center = (xx + 0.5) * scale, xmin = max((int)(center - support + 0.5), 0), count = min((int)(center + support +
 *   0.5), in) - xmin, w[x] = f((x + xmin - center + 0.5) * (1 / filterscale)), summed in order and each divided by the sum when it is
 *   not zero, then (int)(+-0.5 + w * 2^22) with the sign of w.  A horizontal pass writes a uint8 intermediate,
 *   clip8((2^21 + sum in * k) >> 22), a vertical pass over it applies the same expression.  A pass whose axis keeps its size is not
 *   run (Pillow skips it too), and only the intermediate rows and columns the crop window needs are computed.
 * NEAREST is Geometry.c's ImagingScaleAffine: per axis s = in / out, o = s * 0.5, and for each output index in order the source index
 *   is o < 0 ? -1 : (int)o, then o += s (a running sum); an index outside [0, in) leaves the pixel 0.
 *
 * The tables are built on the HOST - HAMMING and LANCZOS go through the C library's sin and cos, the functions Pillow calls - by
 * adain_pil_resize_taps, which needs no device.  Per axis: bounds_host int32 [out_size][2] (first source index, tap count) and
 * taps_host int32 [out_size][ksize] (zero behind the count); `bytes` is the size of both together.  NEAREST: ksize 0, bounds holds
 * the source index and 1 (0 when the index is outside the source), taps_host may be NULL.
 *
 * adain_resize_pil_u8 takes both axes' tables as DEVICE pointers (x: wi -> wo, y: hi -> ho).  src: [n][hi][wi][pixel_bytes] with
 * pixel_bytes 1 (L), 3 (packed RGB) or 4 (Pillow's RGBX storage, 4th byte ignored); dst: the window (crop_y0, crop_x0, crop_h,
 * crop_w) of the ho x wo result, [n][crop_h][crop_w][1] for pixel_bytes 1 and packed RGB [n][crop_h][crop_w][3] otherwise.  The
 * workspace holds the uint8 intermediate (0 bytes, and the pointer unused, when at most one pass runs); any alignment.  ho == hi and
 * wo == wi copies the window.
 * Refused (ADAIN_EINVAL, with a message, before any launch): an unknown filter; pixel_bytes / channels other than 1, 3, 4; n < 1; a
 * side outside [1, 2^24); a shrink factor above 256 on either axis (in > 256 * out: bounds LANCZOS at 1537 taps per axis); a window
 * outside the result; x_ksize / y_ksize other than the sizes' ksize; null pointers; a workspace too small; a result or workspace that
 * overlaps the source, the tables or each other; more than 65535 images or 262140 rows. */
ADAIN_API int adain_pil_resize_taps_bytes(int filter, int in_size, int out_size, int* ksize, size_t* bytes);
ADAIN_API int adain_pil_resize_taps(int filter, int in_size, int out_size, int32_t* bounds_host, int32_t* taps_host);
ADAIN_API int adain_resize_pil_u8_bytes(int n, int hi, int wi, int ho, int wo, int channels, int filter, int crop_y0, int crop_x0, int crop_h,
                                        int crop_w, size_t* workspace_bytes);
ADAIN_API int adain_resize_pil_u8(const uint8_t* src_u8, int pixel_bytes, int n, int hi, int wi, uint8_t* dst_u8, int ho, int wo, int filter,
                                  const int32_t* x_bounds, const int32_t* x_taps, int x_ksize, const int32_t* y_bounds, const int32_t* y_taps,
                                  int y_ksize, int crop_y0, int crop_x0, int crop_h, int crop_w, void* workspace, size_t workspace_bytes,
                                  adain_stream_t stream);

/* ---- one sub-batch of the reference's batch callers in ONE call ---------------------------------------------------------------
 * What adain_inference does between `Image.open` and `save_image` for n decoded frames of one size and one style whose
 * statistics are already known (test.py:203-244 per frame; the callers loop over frames with the same style,
 * video/utils.py:341-350 and Style_3DGS/train.py:101):
 *     ToTensor + vgg(content)                     adain_encode_u8        test.py:203-204, :57 / :76
 *     calc_mean_std(content_f)                    adain_mean_std         function.py:4-12
 *     depth_maps == NULL:  AdaIN*alpha + content_f*one_minus_alpha       test.py:79-80    (adain_blend_alpha; the caller passes
 *                          float(1 - alpha) computed in double, as the reference's Python scalar is)
 *     depth_maps != NULL:  P = strength map of depth_maps[i] [depth_h[i]][depth_w[i]] per frame (adain_strength_map,
 *                          test.py:66-67), AdaIN*(1-P) + content_f*P     test.py:69-70    (adain_blend_pmap); alpha unused
 *     decoder(feat)                               adain_decode           test.py:71 / :81
 *     mask != NULL:  content*(1-m) + out*m with m = nearest(mask.float()) and out = bilinear(out), both to the frame's size
 *                                                                        test.py:222-236  (adain_resize_* + adain_mask_composite)
 *     x*255 + 0.5, clamp, uint8 HWC                adain_quantize_u8      test.py:243-244
 * Every stage runs the kernel of the entry point named beside it with the same arguments, so `out_u8` holds the bytes that
 * sequence of calls gives; the tails are fused with the same arithmetic: without a mask the decoder's last layer quantises its
 * pixels itself (no float image in HBM, no quantiser launch); when decoder output and frame share one size (sides that are multiples of 8) the composite's passes
 * and the quantiser run as ONE kernel with the same arithmetic - reading the mask in place when it has the frame's size too (a
 * mask made from the frame itself), sampling it with the nearest resize's index map when it has another (the guide loop: a view
 * resized to content_size with its mask at the view's own size, Style_3DGS/train.py:97-101).
 * frames HWC uint8 [n][h][w][3]; s_mean / s_std [512]: the style's statistics (adain_encode + adain_mean_std of the style
 * image, once per style); depth_maps / depth_h / depth_w: HOST arrays of n device pointers / sizes; mask [mask_n][mask_c]
 * [mask_h][mask_w], mask_n in {1, n}, mask_c in {1, 3}, uint8 / bool bytes (mask_is_float == 0) or float; out_u8 HWC uint8
 * [n][oh][ow][3] with (oh, ow) = adain_stylize_u8_out_size: the frame's size with a mask, 8hc x 8wc without.  One workspace
 * (adain_stylize_u8_workspace_bytes) holds every intermediate.  21-27 kernel launches, no allocation, no synchronisation.
 * adain_stylize_u8_workspace_bytes contains the encoder's and the decoder's and, like them, answers for the device current on the
 * calling thread. */
ADAIN_API size_t adain_stylize_u8_workspace_bytes(int n, int h, int w, int use_depth, int mask_n, int mask_c, int mask_h, int mask_w,
                                        int mask_is_float);
ADAIN_API void adain_stylize_u8_out_size(int h, int w, int has_mask, int* oh, int* ow);
ADAIN_API int adain_stylize_u8(const uint8_t* frames_nhwc_u8, int n, int h, int w, const float* enc_packed, const float* dec_packed,
                     const float* s_mean, const float* s_std, float alpha, float one_minus_alpha,
                     const float* const* depth_maps_host_array_of_dev_ptrs,
                     const int* depth_h_host, const int* depth_w_host, float depth_offset, float depth_prominence, const void* mask,
                     int mask_is_float, int mask_n, int mask_c, int mask_h, int mask_w, uint8_t* out_u8, void* workspace,
                     size_t workspace_bytes, adain_stream_t stream);

/* adain_stylize_u8 with ONE STYLE PER FRAME: s_mean / s_std are [style_n][512], style_n = 1 (every frame takes row 0: exactly
 * adain_stylize_u8, same bytes) or n (frame i takes row i: the statistics of n styles recoloured for their frames by adain_coral,
 * adain_inference(preserve_color=True) for a sub-batch).  Everything else as adain_stylize_u8; the workspace is the same size.
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.) */
ADAIN_API size_t adain_stylize_u8_ex_workspace_bytes(int n, int h, int w, int use_depth, int mask_n, int mask_c, int mask_h, int mask_w,
                                           int mask_is_float);
ADAIN_API int adain_stylize_u8_ex(const uint8_t* frames_nhwc_u8, int n, int h, int w, const float* enc_packed, const float* dec_packed,
                        const float* s_mean, const float* s_std, int style_n, float alpha, float one_minus_alpha,
                        const float* const* depth_maps_host_array_of_dev_ptrs,
                        const int* depth_h_host, const int* depth_w_host, float depth_offset, float depth_prominence, const void* mask,
                        int mask_is_float, int mask_n, int mask_c, int mask_h, int mask_w, uint8_t* out_u8, void* workspace,
                        size_t workspace_bytes, adain_stream_t stream);

/* adain_stylize_u8_ex with a weighted MIX OF K STYLES per frame in place of one style: (s_mean, s_std, k, weights, weights_n,
 * weights_hw) as adain_blend_mix takes them (s_mean / s_std [k][512]; weights on the device, [weights_n][k][weights_hw] with
 * weights_hw = 1 or hc * wc of adain_encoded_size) where _ex takes (s_mean, s_std, style_n).  `out_u8` holds the bytes that
 * adain_encode_u8 -> adain_mean_std -> adain_blend_mix -> adain_decode -> composite -> adain_quantize_u8 give.  No new intermediate:
 * the workspace is adain_stylize_u8_workspace_bytes'.  (Added without a version change: ADAIN_ABI_VERSION stays 4.) */
ADAIN_API size_t adain_stylize_u8_mix_workspace_bytes(int n, int h, int w, int use_depth, int mask_n, int mask_c, int mask_h, int mask_w,
                                            int mask_is_float);
ADAIN_API int adain_stylize_u8_mix(const uint8_t* frames_nhwc_u8, int n, int h, int w, const float* enc_packed, const float* dec_packed,
                         const float* s_mean, const float* s_std, int k, const float* weights, int weights_n, int weights_hw,
                         float alpha, float one_minus_alpha, const float* const* depth_maps_host_array_of_dev_ptrs,
                         const int* depth_h_host, const int* depth_w_host, float depth_offset, float depth_prominence, const void* mask,
                         int mask_is_float, int mask_n, int mask_c, int mask_h, int mask_w, uint8_t* out_u8, void* workspace,
                         size_t workspace_bytes, adain_stream_t stream);

/* ---- the callers' output files: PIL's Image.fromarray(frame).save(path) for a .jpg path (test.py:243-244 through torchvision's
 * save_image; video/utils.py:352-356 per frame), encoded on the device --------------------------------------------------------------
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.)
 * src: n frames HWC uint8 [n][h][w][c], c = 3 (RGB) or 1 (L) - what adain_stylize_u8, adain_resize_area_u8 and adain_warp_blend_u8
 * write.  Frame i's file - baseline JPEG, JFIF 1.01 header, 4:2:0 chroma for RGB, libjpeg's integer "islow" DCT, the Annex K
 * quantisation tables scaled by `quality` (Pillow's default: 75) and the Annex K Huffman tables: byte for byte what Pillow's default
 * save writes at that quality (established against Pillow 12.2.0 built with libjpeg-turbo; the rules are listed at the top of
 * csrc/jpeg.hip and restated in NumPy in tests/jpeg_ref.py) - lies contiguously at out + i * out_stride and is lengths[i] bytes long
 * (int32, device).  Bytes of `out` behind a file are not written.  Integer arithmetic throughout: a frame's bytes do not depend on
 * the batch, the stream or the device size.
 * adain_jpeg_encode_u8_bytes (host only): *out_stride = the largest file a frame of this shape can have, whatever its content and
 *   quality, so that an overflow is impossible, not detected: a block codes its DC difference in at most 11 + 11 bits (the longest DC
 *   code of category <= 11 plus its bits; 8-bit samples give |DC| <= 1024, so |difference| < 2^11) and each of its 63 AC coefficients
 *   in at most 16 + 10 bits (the longest AC code plus the bits of |AC| < 2^10, which the orthonormal 8 x 8 DCT of samples in
 *   [-128, 127] cannot exceed; a ZRL or the EOB replaces coefficients that would cost more), 22 + 63 * 26 = 1660 bits; B blocks in the
 *   scan (6 per 16 x 16 MCU for RGB, dummy luma blocks included; ceil(h/8) * ceil(w/8) for L) give E = ceil(1660 B / 8) bytes, byte
 *   stuffing at most doubles them, and header (623 bytes RGB, 328 L) and EOI (2) are added: out_stride = header + 2 E + 2.
 *   *workspace_bytes = the coefficients, bit counts, offsets and the unstuffed bit stream of n frames.  Either output may be NULL.
 * Refused with ADAIN_EINVAL before anything is launched: c other than 1 and 3, h or w outside 1..65535, n < 1, quality outside
 * 1..100, n > 65535 (the frames ride in one grid dimension), an out_stride or workspace_bytes below the query's, a workspace that is
 * not 8-byte aligned or `lengths` that is not 4-byte aligned, and a shape whose out_stride would exceed 2^31 - 1 (lengths are int32).
 * 8 kernel launches per call, whatever n. */
ADAIN_API int adain_jpeg_encode_u8_bytes(int n, int h, int w, int c, size_t* out_stride, size_t* workspace_bytes);
ADAIN_API int adain_jpeg_encode_u8(const uint8_t* src_u8, int n, int h, int w, int c, int quality, uint8_t* out, size_t out_stride,
                                   int32_t* lengths, void* workspace, size_t workspace_bytes, adain_stream_t stream);

/* adain_jpeg_encode_u8 with Pillow's `subsampling` and `optimize` keywords: frame i's file is byte for byte what
 * Image.fromarray(frame).save(f, format="JPEG", quality=quality, subsampling=sampling, optimize=optimize) writes (established against
 * Pillow 12.2.0 built with libjpeg-turbo; the rules are listed in csrc/jpeg.hip and restated in NumPy in tests/jpeg_options_ref.py).
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.)
 * sampling: the decoder's encoding - 0: 4:4:4 (8 x 8 MCUs, blocks Y Cb Cr), 1: 4:2:2 (16 x 8 MCUs, Y0 Y1 Cb Cr), 2: 4:2:0 (16 x 16
 *   MCUs, Y00 Y01 Y10 Y11 Cb Cr); SOF0's luma sampling byte is 0x11 / 0x21 / 0x22.  For c = 1 any sampling in 0..2 is accepted and
 *   ignored: the file is the one Pillow writes for an L image without the keyword (given the keyword, Pillow would put the factor into
 *   the grey component's SOF0 byte and change nothing else).
 * optimize: 0 - the Annex K Huffman tables; 1 - libjpeg's two-pass optimize_coding: per frame and table (DC0, AC0 and for RGB DC1, AC1)
 *   the symbols of the scan are counted (64-bit counters), the optimal length-limited code is built on the device, and the file's DHT
 *   segments hold that code with only the symbols that occur, so the header's length varies per frame.
 * (sampling 2, optimize 0) is adain_jpeg_encode_u8: the same bytes, sizes and launches.
 * adain_jpeg_encode_opt_u8_bytes (host only): as adain_jpeg_encode_u8_bytes, an overflow is impossible, not detected.  A block codes its
 *   DC difference in at most L + 11 bits and each of its 63 AC coefficients in at most L + 10 bits, where L bounds a code's length (the
 *   value bits are as derived above: |difference| < 2^11, |AC| < 2^10; a ZRL or the EOB costs at most L bits and stands for at least
 *   one coefficient that is then not coded).  optimize 0: Annex K's tables, 1660 bits as above.  optimize 1: no code of a JPEG Huffman
 *   table is longer than 16 bits, whatever the counts, so (16 + 11) + 63 * (16 + 10) = 1665 bits.  B blocks in the scan - 3 per 8 x 8
 *   MCU for 4:4:4, 4 per 16 x 8 MCU for 4:2:2, 6 per 16 x 16 MCU for 4:2:0, dummy luma blocks included; ceil(h/8) * ceil(w/8) for L -
 *   give E = ceil(bits B / 8) bytes, byte stuffing at most doubles them; an optimal table lists at most the symbols Annex K's does (12
 *   DC categories; 160 run/size pairs, ZRL and EOB), so the header is at most the standard one (623 bytes RGB, 328 L):
 *   out_stride = header + 2 E + 2.  *workspace_bytes = adain_jpeg_encode_u8_bytes' arrays for that B and, for optimize 1, the symbol
 *   counts and code tables of n frames.  Either output may be NULL.
 * Refused with ADAIN_EINVAL before anything is launched: everything adain_jpeg_encode_u8 refuses, sampling outside 0..2, optimize
 * outside 0..1, and an out_stride or workspace_bytes below THIS query's.  Bytes of `out` behind a file are not written.  Nothing is
 * copied to the host and nothing waits; 8 kernel launches per call for optimize 0 and 10 and one memset for optimize 1, whatever n. */
ADAIN_API int adain_jpeg_encode_opt_u8_bytes(int n, int h, int w, int c, int sampling, int optimize, size_t* out_stride,
                                             size_t* workspace_bytes);
ADAIN_API int adain_jpeg_encode_opt_u8(const uint8_t* src_u8, int n, int h, int w, int c, int quality, int sampling, int optimize,
                                       uint8_t* out, size_t out_stride, int32_t* lengths, void* workspace, size_t workspace_bytes,
                                       adain_stream_t stream);

/* adain_jpeg_encode_opt_u8 with Pillow's `progressive` keyword: frame i's file is byte for byte what Image.fromarray(frame).save(f,
 * format="JPEG", quality=quality, subsampling=sampling, progressive=True) writes (established against Pillow 12.2.0 built with
 * libjpeg-turbo; the rules are listed in csrc/jpeg.hip under "progressive files" and restated in tests/jpeg_progressive_encode_ref.py).
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.)
 * The quantised coefficients are adain_jpeg_encode_opt_u8's; the file is SOF2 with libjpeg's jpeg_simple_progression script - 10 scans
 * for RGB (the Cr scans before the Cb scans), 6 for L - and, as libjpeg forces optimize_coding for progressive files, every scan that
 * codes symbols is preceded by the DHT of the optimal table of its own symbol counts: there is no `optimize` argument, Pillow's
 * progressive=True and progressive=True, optimize=True are the same file.  sampling: as above, ignored for c = 1.
 * adain_jpeg_encode_progressive_u8_bytes (host only): an overflow is impossible, not detected.  Every code may be 16 bits long, and a
 *   coefficient counts in every scan that can spend bits on it (a luma AC coefficient in three, a chroma one in two).  Per block of a
 *   scan: the first DC scan 16 + 11 bits, the second 1; a first AC scan over m coefficients 26 (m - 1) + 30 (a code and 10 value bits
 *   each; the 30 are an end-of-band run's code and 14 count bits, which a block writes at most once and only when its last coefficient
 *   is not coded); a later AC scan 17 (m - 1) + 1 + 30 (a code and a sign bit per new coefficient, one correction bit per old one).
 *   B_s blocks in scan s - the DC scans: the MCU order, dummy luma blocks included; a luma AC scan: ceil(h/8) * ceil(w/8); a chroma AC
 *   scan: the MCUs - give E_s = ceil(bits_s B_s / 8) bytes, stuffing at most doubles them, and each scan adds at most 277 bytes per DHT
 *   (two in the first DC scan of an RGB file) and its SOS: out_stride = the header up to SOF2 + sum over the scans + 2.
 *   *workspace_bytes = the coefficients, per block and scan the run state, bit counts and offsets, the scans' unstuffed bit streams and
 *   the symbol counts and code tables of n frames.  Either output may be NULL.
 * Refused with ADAIN_EINVAL before anything is launched: everything adain_jpeg_encode_opt_u8 refuses.  Bytes of `out` behind a file
 * are not written.  Nothing is copied to the host and nothing waits; 13 kernel launches and one memset per call, whatever n.  One of
 * them walks each end-of-band run with one wave, 64 blocks a step (libjpeg cuts a run greedily once it holds more than 937 correction
 * bits, which no parallel scan places): a frame without any detail is one run per scan and one wave walks all its blocks. */
ADAIN_API int adain_jpeg_encode_progressive_u8_bytes(int n, int h, int w, int c, int sampling, size_t* out_stride, size_t* workspace_bytes);
ADAIN_API int adain_jpeg_encode_progressive_u8(const uint8_t* src_u8, int n, int h, int w, int c, int quality, int sampling, uint8_t* out,
                                               size_t out_stride, int32_t* lengths, void* workspace, size_t workspace_bytes,
                                               adain_stream_t stream);

/* ---- PNG output files: the reference's save of a .png path (test.py:243-244, video/utils.py:292-296, train.py:104-114) --------------
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.)
 * src: n frames HWC uint8 [n][h][w][c], c = 3 (colour type 2) or 1 (colour type 0), at any byte address.  Row i of `out`
 * ([n][out_stride] bytes, at any byte address) starts with frame i's file and lengths[i] (int32, 4-byte aligned) is its size: an 8-bit
 * non-interlaced PNG of signature, IHDR, one IDAT and IEND that any reader decodes to the frame's pixels.  The bytes are NOT Pillow's
 * (that would be zlib's sequential matcher); they are a function of the frame and `filter` alone - not of n, the stream or the device
 * - by the rules listed at the top of csrc/png.hip and restated in tests/png_ref.py.  filter: -1 chooses every row's filter by
 * libpng's minimum sum of magnitudes, 0..4 forces None, Sub, Up, Average or Paeth on every row.
 * adain_png_encode_u8_bytes (host only): *out_stride = the largest file a frame of this shape can have; an overflow is impossible, not
 *   detected.  The filtered stream has S = h (w c + 1) bytes in B = ceil(S / 32768) deflate blocks.  Every block is written with the
 *   cheaper of its own Huffman code and the fixed one, so it costs at most what the fixed code costs: 9 bits for a literal at most; a
 *   match (4..258 bytes) at most 8 + 5 + 5 + 13 = 31 bits, less than the 32 its four or more literals would cost at least; 3 header bits
 *   and the 7 of the end-of-block symbol per block.  With the zlib header (2), the Adler-32 (4) and the file's 57 bytes of signature,
 *   IHDR, IDAT frame and IEND: out_stride = 63 + ceil((9 S + 10 B) / 8).  *workspace_bytes = the filtered stream, one 16-bit token per
 *   filtered byte, per block the code tables, bit count and offset, and the zlib stream at its bound, of n frames.  Either output may be
 *   NULL.
 * Refused with ADAIN_EINVAL before anything is launched: null pointers, c outside {1, 3}, h or w outside 1..65535, n outside 1..65535,
 * filter outside -1..4, a frame whose out_stride would pass 2^31 - 1, out_stride or workspace_bytes below the query's, a workspace
 * that is not 8-byte aligned, lengths that is not 4-byte aligned.  Bytes of `out` behind a file are not written.  Nothing is copied
 * to the host and nothing waits; 7 kernel launches and one memset per call, whatever n.
 * What stays with Pillow: 16-bit, palette and RGBA images, interlace, ancillary chunks, compress_level, optimize. */
ADAIN_API int adain_png_encode_u8_bytes(int n, int h, int w, int c, size_t* out_stride, size_t* workspace_bytes);
ADAIN_API int adain_png_encode_u8(const uint8_t* src_u8, int n, int h, int w, int c, int filter /* -1: adaptive */, uint8_t* out,
                                  size_t out_stride, int32_t* lengths, void* workspace, size_t workspace_bytes, adain_stream_t stream);

/* ---- PNG input files decoded on the device, pixel for pixel what Pillow's Image.open gives (train.py:86-115, test.py's content image,
 * video/utils.py's frames) ----------------------------------------------------------------------------------------------------------------
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.)
 * n files of ONE shape: height h, width w, c_file channels (1: colour type 0, 3: colour type 2, 4: colour type 6), 8 bits deep,
 * non-interlaced.  The host walks the chunks (png_file.py does; a file it refuses stays with the host decoder) and hands over
 *   streams, streams_bytes   device memory, any address: per file its IDAT payloads joined - a zlib stream (RFC 1950) whose two header
 *     bytes the host has checked - back to back
 *   offsets   HOST array uint64 [n + 1], read before the call returns: file i's stream is streams[offsets[i] .. offsets[i + 1])
 *   out   HWC uint8 [n][h][w][c_out], any address.  c_out is c_file, or 3: grey is replicated and alpha is dropped, the pixels of
 *     Pillow's convert("RGB") (established against Pillow 12.2.0)
 *   record   device int32 [n][2], 4-byte aligned: file i's status and the deflate blocks it read.  Status 0: decoded; anything else: the
 *     frame's content is unspecified (its writes stay inside out) and the caller decodes the file on the host
 * The rules are RFC 1950 / 1951 in full - stored, fixed and dynamic blocks, the whole 32 KiB window, matches that overlap their own
 * output - and the PNG specification's five filters, restated in tests/png_decode_ref.py; the cores are csrc/png_inflate.h, which
 * compiles for the host as well.  A wave per file inflates (one lane decodes up to 64 tokens, the wave writes them) into the filtered
 * stream h (w c_file + 1) in the workspace and checks the Adler-32; a wave per file unfilters bands of 64 rows as a diagonal wavefront
 * and writes the pixels.  Integer arithmetic throughout: a frame does not depend on the batch, the stream, the device or on what the
 * workspace held.  3 kernel launches and one more per 64 files per call; no copy to the host, no wait.
 * The decoder is total: whatever the bytes, every read stays inside the file's own [offsets[i], offsets[i + 1]), every write inside
 * out, record and the workspace, every loop iteration consumes a bit of the stream or writes a byte, and a damaged file changes
 * nothing about its neighbours in the call.  The statuses, in the order they are looked for: */
#define ADAIN_PNGD_OK 0
#define ADAIN_PNGD_TRUNCATED 1         /* the stream ends early: inside a header, a code, a stored block or the Adler-32 */
#define ADAIN_PNGD_BLOCK_TYPE 2        /* block type 3 */
#define ADAIN_PNGD_STORED_LEN 3        /* a stored block whose LEN is not ~NLEN */
#define ADAIN_PNGD_OVERSUBSCRIBED 4    /* a set of code lengths with more codes than its lengths allow */
#define ADAIN_PNGD_INCOMPLETE 5        /* an incomplete set other than the single one-bit code zlib accepts (a set without codes is accepted too) */
#define ADAIN_PNGD_REPEAT 6            /* a repeat code with nothing to repeat, or one that runs past HLIT + HDIST */
#define ADAIN_PNGD_NO_END_OF_BLOCK 7   /* a dynamic block whose symbol 256 has no code */
#define ADAIN_PNGD_BAD_SYMBOL 8        /* length symbol 286 / 287 or distance symbol 30 / 31 */
#define ADAIN_PNGD_FAR_DISTANCE 9      /* a distance that reaches before the stream's start */
#define ADAIN_PNGD_TOO_MUCH 10         /* more output than h (w c_file + 1) */
#define ADAIN_PNGD_TOO_LITTLE 11       /* less output than that */
#define ADAIN_PNGD_TRAILING 12         /* bytes between the final block and the Adler-32, or behind it */
#define ADAIN_PNGD_ADLER 13            /* the Adler-32 of the output is not the trailer's */
#define ADAIN_PNGD_FILTER 14           /* a row whose filter byte is above 4 */
#define ADAIN_PNGD_UNUSED_CODE 15      /* bits that are no code of an incomplete set that was accepted */
#define ADAIN_PNGD_TOO_MANY_SYMBOLS 16 /* HLIT above 286 or HDIST above 30 */
/* adain_png_decode_u8_bytes (host only): *workspace_bytes = the offsets, 8 bytes per file and the filtered streams of n files; it does
 *   not depend on max_stream_bytes, the longest stream of the call, which is only checked.  The output may be NULL.
 * Refused with ADAIN_EINVAL before anything is launched: a null pointer, c_file outside {1, 3, 4}, a c_out that is neither c_file nor 3,
 * h or w below 1, n outside 1..65535, h (w c_file + 1) of 2^31 or more, offsets that run backwards or leave `streams`, a stream of 2^31
 * bytes or more, a workspace_bytes below the query's, a workspace that is not 8-byte aligned, a record that is not 4-byte aligned.
 * What stays with Pillow: palette, grey + alpha, 1 / 2 / 4 / 16-bit and interlaced files, tRNS, APNG. */
ADAIN_API int adain_png_decode_u8_bytes(int n, int h, int w, int c_file, size_t max_stream_bytes, size_t* workspace_bytes);
ADAIN_API int adain_png_decode_u8(const uint8_t* streams, size_t streams_bytes, const uint64_t* offsets, int n, int h, int w, int c_file,
                                  int c_out, uint8_t* out, int32_t* record, void* workspace, size_t workspace_bytes, adain_stream_t stream);

/* ---- pixel-art palette control: the reference's palette page (gui/second_page.py, MainWindow._convert_image and its helpers) --------
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.)
 * src, out: n frames HWC uint8 [n][h][w][3] at any byte address.  palette: K x 3 uint8 in device memory, 1 <= K <= 256; duplicate
 * entries are legal.  index: NULL, or uint8 [n][h][w] that receives the chosen entry of every pixel.  The rules are listed at the top
 * of csrc/palette.hip and restated in tests/palette_ref.py.
 * The tone step runs in front of every call here, and alone as adain_tone_u8 (there src may be out):
 *   grey != 0: Pillow's convert("L").convert("RGB"), L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 in all three channels
 *     (established against Pillow 12.2.0), then
 *   lut != NULL: uint8 [3][256] in device memory, channel c becomes lut[c][value].  _adjust_brightness_and_contrast is a function of the
 *     channel value alone: the host evaluates the reference's float64 expression on 0..255 and uploads the table.
 * adain_palette_map_u8: one thread per pixel, integer arithmetic, the lowest index among equal distances.
 *   metric 0 ("rgb", _recolor_image's bytes): minimise sum_c ((p_c - P_kc) & 255)^2 - the reference subtracts uint8 from uint8, so
 *     every channel difference wraps modulo 256 before the norm
 *   metric 1 ("nearest", _recolor_image_kd; also what _recolor_image_floyd computes, whose error is read through a view of the pixel
 *     it has just overwritten and is therefore zero): minimise sum_c (p_c - P_kc)^2
 * adain_palette_dither_u8: Floyd-Steinberg error diffusion, the loop _recolor_image_floyd spells out with the error copied before the
 *   pixel is overwritten.  float32, one operation at a time:
 *     v = ((((p + e[y-1][x-1] * 1/16) + e[y-1][x] * 5/16) + e[y-1][x+1] * 3/16) + e[y][x-1] * 7/16), every product rounded before its
 *       add, terms outside the frame left out; v is not clamped
 *     t_k = sqrt((d0 d0 + d1 d1) + d2 d2) correctly rounded, d = P_k - v; the first k with the smallest t_k is chosen (the root, not the
 *       sum, is compared: it merges neighbouring sums); e = v - P_k; the output pixel is P_k
 *   One workgroup per frame; a thread per row of a band of ADAIN_PALETTE_DITHER_BAND rows, row y two columns behind row y - 1, one
 *   barrier per step and w + 2 (rows - 1) steps per band for every thread; no spin-wait, flag or atomic.  A band's last error row
 *   passes to the next band through the workspace.  A frame's bytes depend on the frame, the palette and the tone step alone - not on
 *   n, the stream, the device or what the workspace held.
 * adain_palette_dither_u8_bytes (host only): *workspace_bytes = per frame one error row, w x 3 float.  The output may be NULL.
 * Refused with ADAIN_EINVAL before anything is launched, adain_last_error naming the argument: a null src, palette or out, K outside
 * 1..256, a metric other than 0 and 1, h, w or n below 1, n above 65535, a frame beyond 2^31 - 1 bytes, a null workspace, a
 * workspace_bytes below the query's, a workspace that is not 8-byte aligned.  out must not overlap src partially (map and dither:
 * not at all).  Nothing is copied to the host and nothing waits; one kernel launch per call. */
#define ADAIN_PALETTE_DITHER_BAND 1024
#define ADAIN_PALETTE_METRIC_RGB 0
#define ADAIN_PALETTE_METRIC_NEAREST 1
ADAIN_API int adain_palette_map_u8(const uint8_t* src_u8, int n, int h, int w, const uint8_t* palette, int K, int metric, const uint8_t* lut_or_null,
                                   int grey, uint8_t* out_u8, uint8_t* index_or_null, adain_stream_t stream);
ADAIN_API int adain_tone_u8(const uint8_t* src_u8, int n, int h, int w, const uint8_t* lut_or_null, int grey, uint8_t* out_u8, adain_stream_t stream);
ADAIN_API int adain_palette_dither_u8_bytes(int n, int h, int w, size_t* workspace_bytes);
ADAIN_API int adain_palette_dither_u8(const uint8_t* src_u8, int n, int h, int w, const uint8_t* palette, int K, const uint8_t* lut_or_null, int grey,
                                      uint8_t* out_u8, uint8_t* index_or_null, void* workspace, size_t workspace_bytes, adain_stream_t stream);

/* ---- animated GIF clips: the frame records of the file Pillow's save(save_all=True) writes in the reference (Style_3DGS/render.py:29-33
 * create_gif; video/utils.py:374-392 frames_to_video writes a cv2 video instead) -------------------------------------------------------
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.)
 * index: n palette index planes uint8 [n][h][w] at any byte address - what adain_palette_map_u8 / adain_palette_dither_u8 write - with
 * every index below K.  Row i of `out` ([n][out_stride] bytes, at any byte address) starts with frame i's record and lengths[i] (int32,
 * 4-byte aligned) is its size: graphic control extension (disposal 1, no transparency, delay_cs centiseconds), image descriptor (full
 * frame, no local table, not interlaced), minimum code size m = max(2, ceil(log2 K)), the LZW data in sub-blocks of 255, terminator.
 * The records of a clip back to back between a header with the global colour table and the trailer 3B are an animated GIF any reader
 * plays (gif_file.py builds that file).  The bytes are NOT Pillow's: the indices are cut into segments of ADAIN_GIF_SEGMENT = 2048
 * pixels that each start with CLEAR and an empty dictionary, so that segments are coded side by side; they are a function of the
 * indices, K and delay_cs alone - not of n, the stream, the device or what the workspace held - by the rules listed at the top of
 * csrc/gif.hip and restated in tests/gif_ref.py.
 * adain_gif_encode_u8_bytes (host only): *out_stride = the largest record a frame of this shape can have; an overflow is impossible,
 *   not detected.  The k-th code behind a CLEAR has w(k) bits, the smallest w >= m + 1 with 2^m + 1 + k <= 2^w; W(c) = w(1) + ... + w(c).
 *   A segment of p pixels emits at most p codes (greedy LZW never emits more codes than pixels) and is closed by one more, the next CLEAR
 *   or EOI: at most W(p + 1) bits.  With the first CLEAR's m + 1 bits, D = ceil(((m + 1) + sum over the segments of W(p_s + 1)) / 8)
 *   data bytes at most, and out_stride = 20 + D + ceil(D / 255): 8 + 10 + 1 bytes in front, a length byte per sub-block, the terminator.
 *   *workspace_bytes = 2048 16-bit codes, a count and a bit offset per segment, a bit total and a flag per frame, and the bit stream at
 *   its bound, of n frames.  Either output may be NULL.
 * A frame with an index >= K cannot be coded (the index would collide with CLEAR): lengths[i] = 0 and no byte of its row is written;
 * the other frames of the call are not affected.  What the kernels use as an address is clamped first.
 * Refused with ADAIN_EINVAL before anything is launched, adain_last_error naming the argument: null pointers, K outside 1..256, h or w
 * outside 1..65535, n outside 1..65535, delay_cs outside 0..65535, a frame whose out_stride would pass 2^31 - 1, out_stride or
 * workspace_bytes below the query's, a workspace that is not 8-byte aligned, lengths that is not 4-byte aligned.  Bytes of `out` behind
 * a record are not written.  Nothing is copied to the host and nothing waits; 5 kernel launches and one memset per call, whatever n.
 * A palette chosen from the clip: adain_quantize_palette_u8 below; local colour tables: gif_file.py splices them into these records on the
 * host.  Not built: frame differencing and transparency, interlace, reading GIFs. */
#define ADAIN_GIF_SEGMENT 2048
ADAIN_API int adain_gif_encode_u8_bytes(int n, int h, int w, int K, size_t* out_stride, size_t* workspace_bytes);
ADAIN_API int adain_gif_encode_u8(const uint8_t* index_u8, int n, int h, int w, int K, int delay_cs, uint8_t* out, size_t out_stride,
                                  int32_t* lengths, void* workspace, size_t workspace_bytes, adain_stream_t stream);

/* ---- a palette chosen from the frames themselves: the stage in front of adain_palette_map_u8 / adain_palette_dither_u8 and
 * adain_gif_encode_u8 for a full-colour clip (Style_3DGS/render.py:29-33 create_gif hands Pillow RGB frames, which Pillow quantises to an
 * adaptive palette each; gui/seven_page.py extract_palette) ---------------------------------------------------------------------------
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.  adain_quantize_u8 above is the float -> uint8
 * quantiser of save_image and has nothing to do with this call.)
 * src: n frames HWC uint8 [n][h][w][3] at any byte address.  mode ADAIN_QUANTIZE_GLOBAL: one palette for the n frames, P = 1;
 * ADAIN_QUANTIZE_PER_FRAME: one per frame, P = n.  palettes: uint8 [P][256][3]; used: int32 [P], 4-byte aligned.  Palette p has used[p]
 * <= K colours in its first entries, the entries behind them are zero.  NOT Pillow's palette: a median cut over a 32 x 32 x 32 grid of
 * cells (value >> 3) with integer moments, the box with the largest squared error split at its pixel median along its longest side, every
 * comparison exact; a function of the pixels, K and mode alone - not of the stream, the device or what the workspace held - by the rules
 * listed at the top of csrc/quantize.hip and restated in tests/quantize_ref.py.  Two colours in one cell are merged: a frame with fewer
 * than K non-empty cells gets used < K.
 * adain_quantize_palette_u8_bytes (host only): *workspace_bytes = per palette the five planes of the grid, 32768 x (4 + 4 x 8) bytes.
 * Refused with ADAIN_EINVAL before anything is launched, adain_last_error naming the argument: a null src, palettes or used, K outside
 * 1..256, a mode other than the two, h, w or n below 1, n above 65535, 2^32 or more pixels for one palette (n h w for GLOBAL, h w for
 * PER_FRAME), a null workspace, workspace_bytes below the query's, a workspace that is not 8-byte aligned, used that is not 4-byte
 * aligned, palettes, used or the workspace overlapping src.  Nothing is copied to the host and nothing waits; 3 kernel launches and
 * one memset per call, whatever n.
 * K-MEANS REFINEMENT (added without a version change: no declaration moved or was added).  mode & 0xff is ADAIN_QUANTIZE_GLOBAL or
 * ADAIN_QUANTIZE_PER_FRAME; mode >> 8 is the number of rounds T, 0..ADAIN_QUANTIZE_REFINE_MAX, or-ed on with ADAIN_QUANTIZE_REFINE(T);
 * every other mode is refused as above.  T = 0 is the call described above: the same launches, workspace, palette and used.  With
 * T > 0 the cut's palette P and used = u are refined T times, in integers, by the rules at the top of csrc/quantize_refine.hip, restated
 * in tests/quantize_refine_ref.py:
 *   7.  every pixel goes to the entry i < u with the smallest squared Euclidean distance, the lowest i among equals;
 *   8.  per entry: the count n, the sums S[c], and the far key F = max((d << 24) | (0xFFFFFF - (r << 16 | g << 8 | b))) over its pixels
 *       at distance d: the farthest colour, among equally far ones the smallest r, g, b value;
 *   9.  n > 0: the entry becomes (2 S[c] + n) / (2 n), rounded down; n == 0: it stays;
 *   10. the free slots - i < K with n == 0, ascending: every i >= u and any live entry without a pixel - take, one each, the far colours
 *       of the donors - entries with n > 0 and F >> 24 > 0, by that distance descending, then index ascending - as long as both lists
 *       last; u' = max(u, 1 + the highest slot filled): a palette can at most double per round, so a frame with fewer than K non-empty
 *       cells reaches K colours where it has them;
 *   11. P, u <- P', u'; entries u..255 are zero at the end.
 * The result is a function of the multiset of the pixels, K, T and the mode alone.  A round that changes nothing is a fixed point: T and
 * T + 1 then agree.  The workspace gains per palette the accumulators of rule 8, 256 x 5 x 8 bytes, behind the grids; the call is
 * 3 + 2 T kernel launches and one memset, a chain fixed by the arguments. */
#define ADAIN_QUANTIZE_GLOBAL 0
#define ADAIN_QUANTIZE_PER_FRAME 1
#define ADAIN_QUANTIZE_REFINE_MAX 64
#define ADAIN_QUANTIZE_REFINE(t) ((t) << 8)   /* or-ed onto ADAIN_QUANTIZE_GLOBAL / _PER_FRAME */
ADAIN_API int adain_quantize_palette_u8_bytes(int n, int h, int w, int mode, size_t* workspace_bytes);
ADAIN_API int adain_quantize_palette_u8(const uint8_t* src_u8, int n, int h, int w, int K, int mode, uint8_t* palettes_u8, int32_t* used_i32,
                                        void* workspace, size_t workspace_bytes, adain_stream_t stream);

/* ---- image quality metrics of frames that are already on the device: the scores Style_3DGS/metrics.py computes per view with
 * utils/loss_utils.py ssim (window 11, sigma 1.5) and utils/image_utils.py psnr, and the l1_loss / l2_loss beside them ------------------
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.)
 * adain_image_metrics_u8: a, b are n frames HWC uint8 [n][h][w][c], c = 1 or 3, at any byte address, scaled as to_tensor does
 *   (float(x) / 255.0f, a division).  adain_image_metrics_f32: a, b are contiguous NCHW float32 [n][c][h][w], c in 1..4, 4-byte aligned,
 *   values as given (the reference does not clamp).  a may be b.
 * out: double [n][4], 8-byte aligned; frame i's record is {ssim, mse, l1, psnr}:
 *   ssim: the mean over the frame's h w c samples of the reference's map, ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)
 *     (s1 + s2 + C2)) with C1 = 0.01^2, C2 = 0.03^2, under the float32 window gaussian(11, 1.5) (adain_ssim_window), zero padding of 5,
 *     the window not renormalised at the border (a 1 x 1 frame is legal).  The map is float32, its sum float64.  The window is applied
 *     as a row pass and a column pass, not as the reference's 121-tap product: the values differ from the reference's by less than the
 *     reference's differ from float64 (tests/golden/metrics/noise.json).  Equal frames give exactly 1.
 *   mse, l1: the means of (a - b)^2 and |a - b| in the scale of the scaled samples.  uint8: exact integer sums, then one float64
 *     division by h w c 255^2 and by h w c 255.  float32: float64 sums of the float32 differences' squares and magnitudes.
 *   psnr: 20 log10(1 / sqrt(mse)) in float64; +inf for equal frames.
 * ssim_map: NULL, or float32 of the inputs' layout ([n][h][w][c], or [n][c][h][w]), 4-byte aligned, that receives the map; the records
 *   are the same bits with it and without it.
 * A frame's record and map are a function of its two frames alone - not of n, the stream, the device or what the workspace held: a
 * workgroup takes ADAIN_METRICS_TILE_Y rows of ADAIN_METRICS_TILE_X samples (of the packed row of w c samples for uint8, of one plane
 * for float32), reduces them in a fixed order and leaves one partial record in the workspace; a second kernel adds a frame's partial
 * records in index order.  No float atomics.  The rules are listed at the top of csrc/metrics.hip and restated in tests/metrics_ref.py.
 * adain_image_metrics_*_bytes (host only): *workspace_bytes = 24 bytes per tile of the n frames.  The output may be NULL.
 * adain_ssim_window (host only, no device needed): the eleven float32 weights the kernel uses, bit for bit the reference's.
 * Refused with ADAIN_EINVAL before anything is launched, adain_last_error naming the argument: a null a, b or out, c outside the above,
 * n outside 1..65535, h or w below 1, a frame beyond 2^31 - 1 samples, a null workspace, workspace_bytes below the query's, a workspace
 * or out that is not 8-byte aligned, a ssim_map (or float32 a, b) that is not 4-byte aligned, out, ssim_map or the workspace overlapping
 * a or b.  Nothing is copied to the host and nothing waits; 2 kernel launches per call, whatever n.
 * Not built: windows other than 11, LPIPS.  The backward pass is adain_image_metrics_grad_f32 below. */
#define ADAIN_METRICS_TILE_X 64
#define ADAIN_METRICS_TILE_Y 16
ADAIN_API int adain_image_metrics_u8_bytes(int n, int h, int w, int c, size_t* workspace_bytes);
ADAIN_API int adain_image_metrics_u8(const uint8_t* a_u8, const uint8_t* b_u8, int n, int h, int w, int c, double* out, float* ssim_map_or_null,
                                     void* workspace, size_t workspace_bytes, adain_stream_t stream);
ADAIN_API int adain_image_metrics_f32_bytes(int n, int c, int h, int w, size_t* workspace_bytes);
ADAIN_API int adain_image_metrics_f32(const float* a, const float* b, int n, int c, int h, int w, double* out, float* ssim_map_or_null,
                                      void* workspace, size_t workspace_bytes, adain_stream_t stream);
ADAIN_API int adain_ssim_window(float* out11);

/* ---- the gradient of the float32 scores above: what autograd hands back through Style_3DGS/train.py's loss, (1 - lambda) l1_loss +
 * lambda (1 - ssim), and its l1_loss against the stylised guide views -------------------------------------------------------------------
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.)
 * a, b: contiguous NCHW float32 [n][c][h][w], c in 1..4, 4-byte aligned, as adain_image_metrics_f32 takes them.  a may be b.
 * weights: device double [n][3], 8-byte aligned: row i is the upstream gradient of frame i's {ssim, mse, l1}.
 * grad_a: float32 of the inputs' layout, 4-byte aligned: sample j of frame i receives
 *     weights[i][0] d ssim_i / d a_j  +  weights[i][1] 2 (a_j - b_j) / count  +  weights[i][2] sign(a_j - b_j) / count,   count = c h w,
 *   sign(0) = 0.  With the forward pass's mu1, mu2, e11 = E[a^2], e22 = E[b^2], e12 = E[ab] per sample and A = 2 mu1 mu2 + C1,
 *   B = 2 (e12 - mu1 mu2) + C2, D = mu1^2 + mu2^2 + C1, E = (e11 - mu1^2) + (e22 - mu2^2) + C2, map = A B / (D E):
 *     d_mu1 = 2 mu2 (B - A) / (D E) - map (2 mu1 / D - 2 mu1 / E),   d_e11 = -map / E,   d_e12 = 2 A / (D E)
 *     d ssim_i / d a = ( conv(d_mu1) + 2 a conv(d_e11) + b conv(d_e12) ) / count
 *   where conv is the forward pass's window (symmetric, zero padding of 5, not renormalised: its own adjoint), a row pass and a column
 *   pass of 11 taps in float32.  The window statistics are recomputed from a and b; nothing of a forward call is taken.
 * grad_b: NULL, or the same for b (d_mu2, d_e22 and the same d_e12; the mse and l1 terms change sign).
 * Held, and stated at the top of csrc/metrics.hip:
 *   - a frame's gradient bits are a function of its two frames and its three weights alone - not of n, the frame's index, the stream
 *     or what the workspace held;
 *   - a frame whose three weights are all zero receives zeros (of either sign);
 *   - grad_b of (a, b) is bit for bit grad_a of (b, a) under the same weights, and grad_a is the same bits with and without grad_b;
 *   - equal frames receive exactly zero from the ssim term.
 * Kernels: the forward tile pass with another tail, which writes the derivative planes (3, or 5 with grad_b) into the workspace, and a
 * combine pass of the same tile geometry over three of them per gradient: 2 launches, 3 with grad_b, whatever n.  No float atomics.
 * adain_image_metrics_grad_f32_bytes (host only): *workspace_bytes = (with_grad_b ? 5 : 3) planes of n c h w floats, each rounded up
 * to a multiple of 256 bytes.  The output may be NULL.
 * Refused with ADAIN_EINVAL before anything is launched, adain_last_error naming the argument: a null a, b, weights or grad_a, c outside
 * 1..4, n outside 1..65535, h or w below 1, a frame beyond 2^31 - 1 samples, a null workspace, workspace_bytes below the query's, a
 * workspace or weights that is not 8-byte aligned, a, b, grad_a or grad_b that is not 4-byte aligned, grad_a, grad_b or the workspace
 * overlapping a, b, the weights or each other.  Nothing is copied to the host and nothing waits.
 * Not built: a gradient for uint8 input, other windows, a forward call that saves its planes for this one. */
ADAIN_API int adain_image_metrics_grad_f32_bytes(int n, int c, int h, int w, int with_grad_b, size_t* workspace_bytes);
ADAIN_API int adain_image_metrics_grad_f32(const float* a, const float* b, int n, int c, int h, int w, const double* weights, float* grad_a,
                                           float* grad_b_or_null, void* workspace, size_t workspace_bytes, adain_stream_t stream);

/* ---- the guide-view loss of Style_3DGS/train.py:208-221 and its gradient: l1_loss(image, F.interpolate(to_tensor(guide), size=image's,
 * mode="bilinear", align_corners=False)) against uint8 guide views that stay on the device at their own size ------------------------------
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.)
 * image, grad, resampled: contiguous NCHW float32 [n][3][h][w], 4-byte aligned.  guide: contiguous HWC uint8 [n][gh][gw][3] at any byte
 * address (what Image.convert("RGB") is).  Three channels only.
 * The value of one sample; every line rounds once, in float32:
 *   p = float(u8) / 255.0f, a true division (the rule of adain_u8_to_f32);
 *   per axis ATen's rule: scale = f32(in) / f32(out); r = max(scale * (o + 0.5f) - 0.5f, 0); i0 = min(int(r), in - 1);
 *     i1 = i0 + (i0 < in - 1); l1 = clamp(r - i0, 0, 1); l0 = 1 - l1;
 *   top = lx0 * p[y0][x0] + lx1 * p[y0][x1], bot likewise on row y1, g = ly0 * top + ly1 * bot: the bits adain_u8_to_f32 followed by
 *     adain_resize_bilinear produce; a tap of weight 0 still enters the sum;
 *   d = x - g; term = |d|; sign = x > g ? 1 : x < g ? -1 : d (zero, or an input's NaN).
 * adain_guide_l1_f32: out, device double [n], 8-byte aligned: out[i] = (the float64 sum of frame i's terms) / count, count = 3 h w, one
 *   float64 division: train.py's Ll1 of the frame.  resampled: NULL, or receives g (for tests, and for a caller that wants the picture);
 *   out is the same bits with it and without it.  Two launches whatever n: a tile pass in which a thread takes four outputs of a row in
 *   all three planes and a workgroup of 256 threads leaves one float64 partial in the workspace, reduced in a fixed order (per thread,
 *   across the wave by shuffles, across the waves through LDS), and a finish kernel that adds a frame's partials lane-parallel and then
 *   in a fixed tree.
 * adain_guide_l1_grad_f32: weights, device double [n], 8-byte aligned: the upstream gradient of out[i].  grad sample j of frame i
 *   receives (float)(weights[i] / count) * sign_j, the scalar formed in float64 and rounded once.  One launch; g is recomputed and nothing
 *   of a forward call is taken.  A frame whose weight is zero receives zeros and neither its image nor its guide is read.
 * Both: the image is read (and the gradient written) 16 bytes at a time where w % 4 == 0 and the float buffers are 16-byte aligned, sample
 * by sample otherwise; the guide is gathered from global memory.  No float atomics, spin-waits or flags: a frame's out and grad bits are a
 * function of its image, its guide and its weight alone - not of n, the frame's index, the stream or what the workspace held.  The rules
 * are listed at the top of csrc/guide_loss.hip and restated in tests/guide_loss_ref.py.
 * adain_guide_l1_f32_bytes (host only): *workspace_bytes = 8 bytes per workgroup of the n frames (ceil(h ceil(w / 4) / 256) a frame),
 * rounded up to a multiple of 256 bytes.  The output may be NULL.
 * Refused with ADAIN_EINVAL before anything is launched, adain_last_error naming the argument: a null image, guide, out, weights, grad or
 * workspace (a null resampled is legal), n outside 1..65535, h, w, gh or gw below 1, a frame or a guide beyond 2^31 - 1 samples,
 * workspace_bytes below the query's, a workspace, out or weights that is not 8-byte aligned, image, resampled or grad that is not 4-byte
 * aligned, out, resampled, grad or the workspace overlapping image, guide, weights or each other.  Nothing is copied to the host and
 * nothing waits.
 * Not built: a guide with alpha or one channel, antialias=True, align_corners=True, other interpolation modes, a mask, a gradient to the
 * guide, a forward call that saves its signs for the backward, guides streamed from host memory for scenes that do not fit. */
ADAIN_API int adain_guide_l1_f32_bytes(int n, int h, int w, size_t* workspace_bytes);
ADAIN_API int adain_guide_l1_f32(const float* image, const uint8_t* guide_u8, int n, int h, int w, int gh, int gw, double* out,
                                 float* resampled_or_null, void* workspace, size_t workspace_bytes, adain_stream_t stream);
ADAIN_API int adain_guide_l1_grad_f32(const float* image, const uint8_t* guide_u8, int n, int h, int w, int gh, int gw, const double* weights,
                                      float* grad, adain_stream_t stream);

/* ---- the lossy JPEG round trip without the file: the reference's save and re-read of every stylised frame in front of the temporal
 * recurrence (video/utils.py:261-273) -------------------------------------------------------------------------------------------------
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.)
 * src, dst: n frames HWC uint8 [n][h][w][c], c = 3 (RGB) or 1 (L), at any byte address.  dst frame i holds the pixels Pillow decodes
 * (Image.open(...), mode RGB for c = 3, mode L for c = 1) from the file its Image.fromarray(frame i).save(f, format="JPEG",
 * quality=quality) writes, byte for byte (established against Pillow 12.2.0 built with libjpeg-turbo).  No file is made: entropy coding
 * is lossless, so the decoded pixels are a function of the quantised coefficients adain_jpeg_encode_u8's transform stage computes.  Behind
 * that stage run the coefficient times its quantisation-table entry, libjpeg's integer "islow" inverse DCT (columns, then rows) with its
 * 1024-entry range-limit table, the crop of the luma block grid to h x w, for RGB libjpeg's h2v2 "fancy" chroma upsampling of the
 * ceil(h/2) x ceil(w/2) real chroma samples (plain 2 x 2 replication when w <= 4, as libjpeg does) and its YCbCr -> RGB map.  The rules
 * are listed at the top of csrc/jpeg.hip and restated in NumPy in tests/jpeg_decode_ref.py.  Integer arithmetic throughout: a frame's
 * bytes do not depend on the batch, the stream or the device size.
 * adain_jpeg_roundtrip_u8_bytes (host only): *workspace_bytes = the coefficients (2 bytes per sample of the padded block grid) and the
 *   uint8 Y / Cb / Cr planes of n frames.  The output may be NULL.
 * Refused with ADAIN_EINVAL before anything is launched: a null pointer, c other than 1 and 3, h or w outside 1..65535, n < 1, quality
 * outside 1..100, n > 65535 (the frames ride in one grid dimension), a workspace_bytes below the query's, a workspace that is not
 * 8-byte aligned, and a dst whose n h w c bytes overlap src's.  3 kernel launches per call, whatever n. */
ADAIN_API int adain_jpeg_roundtrip_u8_bytes(int n, int h, int w, int c, size_t* workspace_bytes);
ADAIN_API int adain_jpeg_roundtrip_u8(const uint8_t* src_u8, int n, int h, int w, int c, int quality, uint8_t* dst_u8, void* workspace,
                                      size_t workspace_bytes, adain_stream_t stream);

/* ---- the callers' input files: baseline JPEG files decoded on the device, pixel for pixel what Pillow's Image.open gives ----------------
 * (Added without a version change: nothing existing moved, ADAIN_ABI_VERSION stays 4.)
 * n files of ONE geometry: height h, width w, c components (1: grey, 3: YCbCr) and luma sampling (0: 1 x 1 - 4:4:4 and grey, 1: 2 x 1 -
 * 4:2:2, 2: 2 x 2 - 4:2:0; chroma 1 x 1), 8-bit baseline or extended-sequential Huffman, one interleaved scan, no restart interval.  The
 * host walks the markers (jpeg_file.py does; a file it refuses stays with the host decoder) and hands over
 *   files, files_bytes   device memory that holds the files' bytes, at any address
 *   segment_offsets, segment_lengths   HOST arrays [n]: where file i's entropy-coded segment (behind SOS, in front of EOI, stuffed) lies in
 *     `files` and how long it is; they are read before the call returns
 *   blobs   device memory, n x 3848 bytes, any address: file i's tables - four Huffman tables DC0, DC1, AC0, AC1 of 912 bytes (look[256]
 *     uint16: (code length << 8) | symbol for the next 8 bits of the stream, 0: none that short; maxcode[18] int32 by length, -1: none;
 *     valoff[18] int32: index of the length's first symbol minus its first code; val[256] uint8: HUFFVAL), q[3][64] uint8: each
 *     component's quantisation table in natural order, sel[8] uint8: the DC table of components 0..2, the AC table of components 0..2, 0, 0
 *   dst   HWC uint8 [n][h][w][c], any address: frame i = np.asarray(Image.open(file i)) (established against Pillow 12.2.0 built with
 *     libjpeg-turbo; the rules are listed in csrc/jpeg_decode.hip and restated in tests/jpeg_file_ref.py)
 *   record   device int32 [n][2]: file i's status and the rounds its entropy decode took.  Status 0: decoded.  Non-zero: the entropy data
 *     did not decode to exactly the expected number of blocks ending inside the last byte, or held a code or value no 8-bit baseline
 *     encoder writes; that frame's content is then unspecified (its writes stay inside dst) and the caller decodes the file on the host
 *   chunk_bits   the bits of one subsequence of the parallel entropy decode: 0 for the default (1024), else a multiple of 32 from 32 up.
 *     The pixels do not depend on it, nor on the batch, the stream or the device: integer arithmetic throughout.
 * The entropy decode trusts no self-synchronisation: the exit states of the subsequences are iterated to their fixed point, which is the
 * sequential decoder's, in at most (subsequences + 1) rounds inside one workgroup per file.  No copy to the host, no wait.
 * adain_jpeg_decode_u8_bytes (host only): *workspace_bytes for n files whose longest segment is max_segment_bytes.  The output may be NULL.
 * Refused with ADAIN_EINVAL before anything is launched: a null pointer, c other than 1 and 3, sampling outside 0..2 or not 0 for
 * c = 1, h or w outside 1..65535, n outside 1..65535, a chunk_bits that is neither 0 nor a multiple of 32 from 32 up, a segment that
 * leaves `files` or is 2^28 bytes or longer, a workspace_bytes below the query's for the longest segment, a workspace that is not
 * 8-byte aligned or a record that is not 4-byte aligned.  7 kernel launches, one memset and one more launch per 64 files per call.
 *
 * adain_jpeg_decode_restart_u8 / _bytes (added without a version change): the same call for files that carry a restart interval,
 * restart_interval = the DRI segment's Ri in MCUs, ONE value per call, 0..65535 (anything else: ADAIN_EINVAL before any launch).  0 means
 * "no restart interval": that is adain_jpeg_decode_u8, which is this entry at 0 with an unchanged workspace query.  With Ri > 0 the
 * segments still run from behind SOS to EOI and hold their FF D0..D7 markers; the device finds and removes them itself while it
 * unstuffs, keeps each interval's first stream byte in the workspace, decodes every interval from its own byte-aligned all-zero state
 * (subsequences are cut per interval, so the rounds are the largest count any interval needs) and restarts the DC sums at every
 * interval's first MCU.  nint = ceil(MCUs / Ri); the status is also non-zero when the markers found are not nint - 1 or marker m is not
 * FF D(m mod 8) - no resynchronisation is tried, such a file goes to the host - and when any interval has damage, too few blocks or a
 * last block that does not end inside the interval's last byte.  Whatever the bytes, the writes stay inside dst, record and the
 * workspace.  The rules: csrc/jpeg_decode.hip, restated in tests/jpeg_restart_ref.py.  The same launches per call as above. */
ADAIN_API int adain_jpeg_decode_restart_u8_bytes(int n, int h, int w, int c, int sampling, int restart_interval, size_t max_segment_bytes,
                                                 int chunk_bits, size_t* workspace_bytes);
ADAIN_API int adain_jpeg_decode_restart_u8(const uint8_t* files, size_t files_bytes, const uint8_t* blobs, int n, int h, int w, int c,
                                           int sampling, int restart_interval, const uint64_t* segment_offsets,
                                           const uint32_t* segment_lengths, uint8_t* dst_u8, int32_t* record, void* workspace,
                                           size_t workspace_bytes, int chunk_bits, adain_stream_t stream);
ADAIN_API int adain_jpeg_decode_u8_bytes(int n, int h, int w, int c, int sampling, size_t max_segment_bytes, int chunk_bits,
                                         size_t* workspace_bytes);
ADAIN_API int adain_jpeg_decode_u8(const uint8_t* files, size_t files_bytes, const uint8_t* blobs, int n, int h, int w, int c, int sampling,
                                   const uint64_t* segment_offsets, const uint32_t* segment_lengths, uint8_t* dst_u8, int32_t* record,
                                   void* workspace, size_t workspace_bytes, int chunk_bits, adain_stream_t stream);

/* adain_jpeg_decode_progressive_u8 / _bytes (added without a version change): n 8-bit progressive Huffman (SOF2) files of ONE geometry
 * and ONE scan script -> the same dst and record as above.  A complete progressive file holds the quantised coefficients of its
 * sequential twin and Pillow's pixels are a function of those alone, so behind the scans the same back half runs.
 *   nscans, scans   1..32 scans; scans is a HOST array int32 [nscans][8], read before the call returns: the scan's number of components,
 *     their indices in the frame (three entries, unused ones ignored), Ss, Se, Ah, Al.  A DC scan has Ss = Se = 0 and either all components
 *     of the frame in frame order (interleaved, in the MCU order above) or one; an AC scan has 1 <= Ss <= Se <= 63 and one component; a
 *     one-component scan covers that component's own block raster, ceil(ceil(w Hi / Hmax) / 8) blocks a row.  Ah = 0 is a first scan,
 *     Ah > 0 a refinement; Ah and Al are 0..13.  Anything else: ADAIN_EINVAL before any launch.  The order of the scans is the file's.  The
 *     host checks the script (jpeg_file.py does: every coefficient begins with Ah = 0, is refined one bit at a time and ends at Al = 0;
 *     no restart interval); a script that breaks those rules gives unspecified pixels, inside dst.
 *   segment_offsets, segment_lengths   HOST arrays [n][nscans]: file i's scan k lies at segment_offsets[i nscans + k] of `files` (behind
 *     its SOS, up to the next marker, stuffed)
 *   blobs   device memory, [n][nscans] x 3848 bytes in the layout above: the Huffman tables in force at that scan's SOS, sel[] per frame
 *     component (the entries of components the scan does not hold are ignored), and in every blob the frame's quantisation tables
 *   record   status and the rounds SUMMED over the file's Huffman-coded scans (a DC refinement has no code and takes none)
 * Every Huffman-coded scan is decoded by the scheme above - subsequences of chunk_bits bits, exit states iterated to the fixed point in
 * at most (subsequences + 1) rounds, then a parallel write pass - one scan after the other in file order.  An AC refinement's state
 * carries the block it is in, because the bits a block takes depend on which of its coefficients earlier scans made non-zero; that
 * history is taken as one 64-bit mask per block before the scan is settled.  Status non-zero: a code in no table, a size that is illegal
 * for the scan kind (DC above 11, AC above 10, a refinement's above 1), a coefficient index past Se, a value that is no int16, a final
 * DC term outside -2047..2047, a scan with fewer blocks than it covers or whose last block does not end inside its segment's last
 * byte, a scan that did not settle.  Whatever the bytes, the writes stay inside dst, record and the workspace and the kernels end.
 * adain_jpeg_decode_progressive_u8_bytes (host only): *workspace_bytes for n files of nscans scans whose longest scan segment is
 * max_segment_bytes.  Refused as above, and: nscans outside 1..32, a scan that breaks the rules of `scans`.  Launches per call:
 * ceil(n nscans / 64) + 1 + one memset, per scan 3 (DC first), 1 (DC refinement), 2 (AC first) or 3 (AC refinement), and 3 more.  The
 * rules: csrc/jpeg_decode.hip, restated in tests/jpeg_progressive_ref.py. */
ADAIN_API int adain_jpeg_decode_progressive_u8_bytes(int n, int h, int w, int c, int sampling, int nscans, size_t max_segment_bytes,
                                                     int chunk_bits, size_t* workspace_bytes);
ADAIN_API int adain_jpeg_decode_progressive_u8(const uint8_t* files, size_t files_bytes, const uint8_t* blobs, int n, int h, int w, int c,
                                               int sampling, int nscans, const int32_t* scans, const uint64_t* segment_offsets,
                                               const uint32_t* segment_lengths, uint8_t* dst_u8, int32_t* record, void* workspace,
                                               size_t workspace_bytes, int chunk_bits, adain_stream_t stream);

/* ---- layout changes at the boundary ([n][c][hw] <-> [n][hw][c]) ------------------------------------------ */
ADAIN_API int adain_nhwc_to_nchw(const float* in, float* out, int n, int c, int hw, adain_stream_t stream);
ADAIN_API int adain_nchw_to_nhwc(const float* in, float* out, int n, int c, int hw, adain_stream_t stream);

/* ---- one generic 3x3 layer in the form the schedules run (unit tests, profiling) ---------------------------------
 * ReflectionPad2d(1) + Conv2d(cin, cout, 3) [+ ReLU] on NHWC as Winograd F(4,3) x F(2,3): 4 x 2 output tiles, 3 multiplies per
 * output instead of 9 (fp32 rounding error ~5x the direct form's, ~1e-6 relative per layer).  The nearest-2x upsample of the
 * producer may be fused into the input gather (src_mode ADAIN_SRC_UP2X) and the ceil-mode max-pool behind the layer into the
 * epilogue (pool_out != 0: out is [n][ceil(h/2)][ceil(w/2)][cout]).  (h, w) = conv output size before any output pool;
 * (hs, ws) = source size.  Weights packed by adain_conv3x3_wino4_pack, 24 floats per (cin, cout) pair; cin % 16 == 0,
 * cout % 32 == 0; persistent kernel when the launch has >= 2 tiles per resident workgroup.  `form` must be 5 (the other forms -
 * F(2x2,3x3) and the direct implicit GEMM - are retired). */
ADAIN_API size_t adain_conv3x3_wino4_packed_floats(int cin, int cout);
ADAIN_API int adain_conv3x3_wino4_pack(const float* w_oihw, float* packed, int cin, int cout, adain_stream_t stream);
ADAIN_API int adain_conv3x3_wino(const float* in_nhwc, float* out_nhwc, const float* packed_w, const float* bias, int n, int h,
                       int w, int hs, int ws, int cin, int cout, int src_mode, int relu, int pool_out, int form,
                       adain_stream_t stream);

/* The same layer (form 5) as ADAIN_SCHEDULE_LATENCY runs it, whatever the calling thread's schedule: split along cin when the launch
 * has fewer tiles than compute units.  *_workspace_bytes = the partial-sum slabs that launch needs (S x n x h x w x cout floats;
 * 0: it would not be split, and adain_conv3x3_wino4_split then is adain_conv3x3_wino).  The query answers for the device current on
 * the calling thread, whose compute units decide the split.  For unit tests and the per-layer error probe
 * (tools/probes/wino_error_gpu.py). */
ADAIN_API size_t adain_conv3x3_wino4_split_workspace_bytes(int n, int h, int w, int cin, int cout);
ADAIN_API int adain_conv3x3_wino4_split(const float* in_nhwc, float* out_nhwc, const float* packed_w, const float* bias, int n, int h,
                              int w, int hs, int ws, int cin, int cout, int src_mode, int relu, int pool_out, void* workspace,
                              size_t workspace_bytes, adain_stream_t stream);

/* The decoder's up layers as the schedules run them: nearest-2x upsample + ReflectionPad2d(1) + Conv2d(cin, cout, 3) [+ ReLU] on NHWC,
 * computed as four 2 x 2 phase convolutions of the source (pixels (2y + py, 2x + px)) in Winograd F(5,2) x F(3,2), 4 of the 5 rows
 * kept: 2 multiplies per output instead of 3.  in: [n][hs][ws][cin]; out: [n][2 hs][2 ws][cout].  Weights packed by adain_conv3x3_up2x_poly_pack, 96 floats per
 * (cin, cout) pair; cin % 16 == 0, cout % 32 == 0, hs, ws >= 1.  For unit tests and profiling. */
ADAIN_API size_t adain_conv3x3_up2x_poly_packed_floats(int cin, int cout);
ADAIN_API int adain_conv3x3_up2x_poly_pack(const float* w_oihw, float* packed, int cin, int cout, adain_stream_t stream);
ADAIN_API int adain_conv3x3_up2x_poly(const float* in_nhwc, float* out_nhwc, const float* packed_w, const float* bias, int n, int hs,
                                      int ws, int cin, int cout, int relu, adain_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADAIN_HIP_H */
