// Shared declarations for the gfx950 AdaIN kernels (internal; the public C ABI is include/adain_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/adain_hip.h"

namespace adain {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;

// Source-gather modes of the 3x3 convolution's input (fused into the LDS staging):
//   DIRECT   : conceptual input == source tensor
//   UP2X     : conceptual input == nearest 2x upsample of the source, gathered (adain_conv3x3_wino; net.py:10,23,30)
//   POOL2    : conceptual input == MaxPool2d(2,2,ceil_mode=True) of the source (net.py:46,53,66).  No launcher takes it
//              (check_wino4_shape refuses it): the encoder fuses its pools into the PRODUCER's epilogue (ConvArgs::pool_out).
//              The value stays, as ADAIN_SRC_POOL2 does in the public header.
//   UP2X_POLY: UP2X computed as four 2x2 phase convolutions of the source (conv_wino4.hip, W4P; the decoder's up layers)
enum SrcMode { SRC_DIRECT = 0, SRC_UP2X = 1, SRC_POOL2 = 2, SRC_UP2X_POLY = 3 };

struct ConvArgs {
    const float* in;    // NHWC source  [n][Hs][Ws][cin]
    float* out;         // NHWC output  [n][H][W][cout]
    const float* wpk;   // packed weights (pack_wino4_kernel layout)
    const float* bias;  // [cout]
    int n, H, W;        // output (== conceptual input) spatial size
    int Hs, Ws;         // source spatial size
    int cin, cout;
    int relu;
    int pool_out;       // 1: write only MaxPool2d(2,2,ceil_mode=True)(output), [n][ceil(H/2)][ceil(W/2)][cout]
    int tiles_x, tiles_y;
    // cin split of the F(4,3) x F(2,3) one-tile form (set by launch_conv3x3_wino4 only): workgroups per (tile, channel tile),
    // input channels per workgroup, floats between the partial-sum slabs that `out` then points at
    int ksplit, cin_sub;
    size_t slab_stride;
};

// Partial-sum slabs for a cin-split launch of the F(4,3) x F(2,3) kernel (caller-owned workspace; slab == nullptr: never split).
struct SplitWs {
    float* slab;
    size_t floats;
};

// One (source, output) tensor pair of a multi-segment launch of the persistent F(4,3) x F(2,3) kernel: the segments of one
// launch share the layer (weights, bias, cin, cout, source mode, ReLU, output pool) and differ in size and addresses.
struct ConvSeg {
    const float* in;    // NHWC source  [n][Hs][Ws][cin]
    float* out;         // NHWC output  [n][H][W][cout]   (pooled size when the layer's pool_out is set)
    int n, H, W, Hs, Ws;
    int tiles_x, tiles_y;
    int item0;          // first item (tile x channel tile) of this segment in the launch's list
};
constexpr int MAX_CONV_SEGS = 4;
struct ConvSegs {
    int count;
    int ctg;            // channel tiles per group of the persistent walk (divides cout / 32): see conv3x3_wino4_kernel
    ConvSeg s[MAX_CONV_SEGS];
};

// thread-local error text for adain_last_error()
void set_error(const char* fmt, ...);

// ---- scratch memory of a call ("Workspaces") ------------------------------------------------------------------------------
// Every block of a workspace, a pyramid or a packed network starts on a multiple of 256 bytes.
constexpr size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
// Lays blocks out one behind the other: take() returns the block's offset and moves on to the next multiple of 256 bytes, so that
// `at` is the size of everything taken so far.  A call's layout function is the one place that takes its blocks; its size query
// returns the layout's total and its launcher reads the layout's offsets.
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = at; at = align256(at + bytes); return o; }
};
// The one refusal of a launcher's workspace: null, shorter than its layout's total, or (align > 1) not aligned for the layout's types.
inline int check_workspace(const char* who, const void* ptr, size_t have_bytes, size_t need_bytes, size_t align) {
    if (!ptr) set_error("%s: the workspace is a null pointer", who);
    else if (have_bytes < need_bytes) set_error("%s: workspace too small (%zu < %zu bytes)", who, have_bytes, need_bytes);
    else if (align > 1 && (uintptr_t)ptr % align) set_error("%s: the workspace must be %zu-byte aligned", who, align);
    else return 0;
    return ADAIN_EINVAL;
}

// launchers (conv_edge.hip)
int launch_pack_conv_first(const float* w0, const float* b0, const float* w1, const float* b1, float* packed,
                           float* bias_out, hipStream_t s);
int launch_pack_conv_last(const float* w, float* packed, hipStream_t s);
// Compute units of the current device (cached per device id; 0 on failure).  Sizes the persistent kernels' grids.
inline int device_cu_count() {
    static int cached[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    if (!cached[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
        cached[dev] = n;
    }
    return cached[dev];
}

// conv_wino4.hip: F(4,3) x F(2,3) form (its own packed-weight layout, 24 floats per weight pair)
int launch_pack_wino4(const float* w_oihw, float* packed, int cin, int cout, hipStream_t s);
// split: workspace for the cin split of a launch too small to give every compute unit a tile (see wino4_split_floats); without
// one the launch is never split
int launch_conv3x3_wino4(const ConvArgs& a, int src_mode, hipStream_t s, SplitWs split = SplitWs{nullptr, 0});
// the same layer over `count` tensor pairs (sizes / addresses from segs[i]: in, out, n, H, W, Hs, Ws; the rest from `layer`):
// one persistent launch whose tile list covers every segment when there is enough work, one launch per segment otherwise
// (split[i]: segment i's slab workspace for that case, or nullptr)
int launch_conv3x3_wino4_multi(const ConvArgs& layer, const ConvSeg* segs, int count, int src_mode, hipStream_t s,
                               const SplitWs* split = nullptr);
// floats of slab workspace a launch of this layer over n images of H x W (conv output size) needs to be split; 0: it would not be
size_t wino4_split_floats(int n, int H, int W, int cin, int cout);
// persistent-grid rounds one image of a layer is worth (the schedules of api.hip)
double wino4_rounds_per_image(int H, int W, int cout);
// the nearest-2x-upsample layer as four phase convolutions of the source (4 x 24 floats per (cin, cout) pair; see W4P)
int launch_pack_up2x_poly(const float* w_oihw, float* packed, int cin, int cout, hipStream_t s);
int launch_conv3x3_up2x_poly(const ConvArgs& a, hipStream_t s);
// img: NCHW float [n][3][H][W], or (u8 != 0) HWC uint8 [n][H][W][3] converted as ToTensor does (v / 255)
int launch_conv_first(const void* img, int u8, float* out_nhwc, const float* packed, const float* bias, int n, int H,
                      int W, hipStream_t s);
// out_u8 != nullptr: the image is written as save_image's uint8 HWC [n][H][W][3] instead of NCHW float (out_nchw is then unused)
int launch_conv_last(const float* in_nhwc, float* out_nchw, const float* packed, const float* bias, int n, int H,
                     int W, hipStream_t s, uint8_t* out_u8 = nullptr);

// stats.hip
int launch_mean_std(const float* feat, int nhwc, int n, int c, int hw, float eps, float* mean, float* std_,
                    void* workspace, size_t ws_bytes, hipStream_t s);
size_t mean_std_workspace_bytes(int nhwc, int n, int c, int hw);
// What a blend is styled with: s_mean / s_std hold k rows of c statistics.
//   weights == nullptr: k = 1, the one style of every frame or (per_frame) frame i's row i
//   weights != nullptr: the k rows are shared by all frames and mixed by weights [weights_n][k][weights_hw] on the device
//                       (weights_n 1 | n, weights_hw 1 | hw: scalars or per-pixel maps); never with per_frame
constexpr int MIX_MAX_STYLES = 16;   // ADAIN_MIX_MAX_STYLES
struct StyleTerm {
    const float *s_mean, *s_std;
    int k, per_frame;
    const float* weights;
    int weights_n, weights_hw;
};
// How strongly: out = styled * alpha + x * one_minus_alpha, or with pmap [pmap_n][hw] (pmap_n 1 | n) styled * (1 - P) + x * P
struct BlendTerm {
    float alpha, one_minus_alpha;
    const float* pmap;
    int pmap_n;
};
// host only, no HIP call: the argument rules of every blend; what: the entry's name for the error text
int check_adain_blend(const char* what, int nhwc, int n, int c, int hw, const StyleTerm& style, const BlendTerm& blend);
int launch_adain_blend(const float* content, int nhwc, int n, int c, int hw, const float* c_mean, const float* c_std, const StyleTerm& style,
                       const BlendTerm& blend, float* out, hipStream_t s);

// pixel.hip
int launch_strength_map(const float* depth, int h0, int w0, int hc, int wc, float offset, float prominence,
                        float* pmap, void* workspace, size_t ws_bytes, hipStream_t s);
size_t strength_map_workspace_bytes(int hc, int wc);
int launch_resize_bilinear(const float* in, float* out, int planes, int hi, int wi, int ho, int wo, hipStream_t s);
int launch_resize_nearest(const float* in, float* out, int planes, int hi, int wi, int ho, int wo, hipStream_t s);
int launch_mask_composite(const float* content, const float* stylized, const float* mask, int mask_c, int mask_n,
                          float* out, int n, int c, int hw, hipStream_t s);
int launch_warp_blend_u8(const uint8_t* cur, const uint8_t* prev, const float* flow, uint8_t* out, int h, int w, int c,
                         float alpha, float one_minus_alpha, hipStream_t s);
int launch_quantize_u8(const float* in_nchw, uint8_t* out_nhwc, int n, int c, int h, int w, hipStream_t s);
int launch_u8_to_f32(const uint8_t* in_nhwc, float* out_nchw, int n, int c, int h, int w, hipStream_t s);
int launch_resize_area_u8(const uint8_t* in, uint8_t* out, int n, int hi, int wi, int c, int ho, int wo, hipStream_t s);
int launch_composite_quantize_u8(const uint8_t* content_nhwc, const float* stylized_nchw, const void* mask, int mask_is_float,
                                 int mask_c, int mask_n, uint8_t* out_nhwc, int n, int hw, hipStream_t s);
int launch_composite_quantize_u8_nearest(const uint8_t* content_nhwc, const float* stylized_nchw, const void* mask, int mask_is_float,
                                         int mask_c, int mask_n, int mh, int mw, uint8_t* out_nhwc, int n, int h, int w, hipStream_t s);
int launch_mask_to_f32(const uint8_t* in, float* out, size_t total, hipStream_t s);
int launch_nhwc_to_nchw(const float* in, float* out, int n, int c, int hw, hipStream_t s);
int launch_nchw_to_nhwc(const float* in, float* out, int n, int c, int hw, hipStream_t s);

// resample.hip: PIL.Image.resize(size, BILINEAR) on uint8 RGB, bit-exact (Pillow's ImagingResample)
size_t resize_pil_workspace_bytes(int hi, int wi, int ho, int wo);
int launch_resize_pil_bilinear_u8(const uint8_t* in, int pixel_bytes, int n, int hi, int wi, uint8_t* out, int ho, int wo, int y0, int x0, int ch,
                                  int cw, void* workspace, size_t ws_bytes, hipStream_t s);

// resample_filters.hip: PIL.Image.resize for all six filters on uint8 L / RGB, bit-exact: tap tables built on the host (pil_taps.h),
// Pillow's two passes on the device; the launcher refuses everything itself
int pil_resize_taps_bytes(int filter, int in_size, int out_size, int* ksize, size_t* bytes);
int pil_resize_taps(int filter, int in_size, int out_size, int32_t* bounds, int32_t* taps);
int resize_pil_u8_bytes(int n, int hi, int wi, int ho, int wo, int channels, int filter, int y0, int x0, int ch, int cw, size_t* workspace_bytes);
int launch_resize_pil_u8(const uint8_t* src, int pixel_bytes, int n, int hi, int wi, uint8_t* dst, int ho, int wo, int filter, const int32_t* x_bounds,
                         const int32_t* x_taps, int x_ksize, const int32_t* y_bounds, const int32_t* y_taps, int y_ksize, int y0, int x0, int ch, int cw,
                         void* workspace, size_t workspace_bytes, hipStream_t s);

// flow.hip: Farneback dense optical flow (OpenCV's calcOpticalFlowFarneback, flags 0) and the video callers' frame preparation
int launch_flow_gray_u8(const uint8_t* rgb, int n, int hi, int wi, uint8_t* gray, int ho, int wo, hipStream_t s);
int farneback_levels(int h, int w, double pyr_scale, int levels, int* out_levels, int* sizes_wh, int* ksizes, double* sigmas);
size_t farneback_pyramid_bytes(int h, int w, double pyr_scale, int levels);
size_t farneback_workspace_bytes(int h, int w);
int launch_farneback_expand(const uint8_t* gray, int h, int w, double pyr_scale, int levels, int poly_n, double poly_sigma,
                            float* pyramid, void* ws, size_t ws_bytes, hipStream_t s);
int launch_farneback_flow(const float* pyr_prev, const float* pyr_next, int h, int w, double pyr_scale, int levels, int winsize,
                          int iterations, int flags, float* flow_out, void* ws, size_t ws_bytes, hipStream_t s);

// tvl1.hip: Dual TV-L1 dense optical flow (OpenCV's contrib DualTVL1OpticalFlow, CPU path)
int tvl1_scales(int h, int w, const ::adain_tvl1_params* p, int* out_nscales, int* sizes_wh);
size_t tvl1_frame_bytes(int h, int w, const ::adain_tvl1_params* p);
size_t tvl1_workspace_bytes(int h, int w, int npairs, const ::adain_tvl1_params* p);
int launch_tvl1_prepare(const uint8_t* gray, int n, int h, int w, const ::adain_tvl1_params* p, float* prep, hipStream_t s);
int launch_tvl1_flow(const float* const* prev, const float* const* next, int npairs, int h, int w, const ::adain_tvl1_params* p, float* flows, int* iters,
                     void* ws, size_t ws_bytes, hipStream_t s);

// jpeg.hip: baseline JPEG files, byte for byte Pillow's default save (the rules: top of jpeg.hip, tests/jpeg_ref.py)
// sampling 0 / 1 / 2 (4:4:4, 4:2:2, 4:2:0), optimize 0 / 1 (a frame's own Huffman tables): Pillow's save with those keywords
// (tests/jpeg_options_ref.py); (2, 0) is the default file.  who: the entry's name in front of its error messages
int jpeg_encode_bytes(const char* who, int n, int h, int w, int c, int sampling, int optimize, size_t* out_stride, size_t* workspace_bytes);
int launch_jpeg_encode_u8(const char* who, const uint8_t* src, int n, int h, int w, int c, int quality, int sampling, int optimize, uint8_t* out,
                          size_t out_stride, int32_t* lengths, void* workspace, size_t workspace_bytes, hipStream_t s);
// the progressive file Pillow's save(progressive=True) writes (the rules: jpeg.hip, "progressive files"; tests/jpeg_progressive_encode_ref.py)
int jpeg_encode_progressive_bytes(int n, int h, int w, int c, int sampling, size_t* out_stride, size_t* workspace_bytes);
int launch_jpeg_encode_progressive_u8(const uint8_t* src, int n, int h, int w, int c, int quality, int sampling, uint8_t* out, size_t out_stride, int32_t* lengths,
                                      void* workspace, size_t workspace_bytes, hipStream_t s);
// the pixels Pillow decodes from that file, without the file (the rules: top of jpeg.hip, tests/jpeg_decode_ref.py)
int jpeg_roundtrip_bytes(int n, int h, int w, int c, size_t* workspace_bytes);
int launch_jpeg_roundtrip_u8(const uint8_t* src, int n, int h, int w, int c, int quality, uint8_t* dst, void* workspace, size_t workspace_bytes, hipStream_t s);
// jpeg_decode.hip: a baseline file's entropy-coded segment -> the pixels Pillow decodes from the file (the rules: top of jpeg_decode.hip,
// tests/jpeg_file_ref.py)
// restart_interval: MCUs per restart interval, 0 for a file without one (tests/jpeg_restart_ref.py)
int jpeg_decode_bytes(int n, int h, int w, int c, int sampling, int restart_interval, size_t max_segment_bytes, int chunk_bits, size_t* workspace_bytes);
int launch_jpeg_decode_u8(const uint8_t* files, size_t files_bytes, const uint8_t* blobs, int n, int h, int w, int c, int sampling, int restart_interval,
                          const uint64_t* seg_offsets, const uint32_t* seg_lengths, uint8_t* dst, int32_t* record, void* workspace, size_t workspace_bytes,
                          int chunk_bits, hipStream_t s);
// the scans of a progressive (SOF2) file -> the same pixels (the rules: jpeg_decode.hip, tests/jpeg_progressive_ref.py); scans: int32 [nscans][8] =
// components, their frame indices (3), Ss, Se, Ah, Al; seg_offsets, seg_lengths and blobs are [n][nscans]
int jpeg_decode_progressive_bytes(int n, int h, int w, int c, int sampling, int nscans, size_t max_segment_bytes, int chunk_bits, size_t* workspace_bytes);
int launch_jpeg_decode_progressive_u8(const uint8_t* files, size_t files_bytes, const uint8_t* blobs, int n, int h, int w, int c, int sampling, int nscans,
                                      const int32_t* scans, const uint64_t* seg_offsets, const uint32_t* seg_lengths, uint8_t* dst, int32_t* record, void* workspace,
                                      size_t workspace_bytes, int chunk_bits, hipStream_t s);

// png.hip: PNG files any reader decodes to the frame (the rules: top of png.hip, tests/png_ref.py); filter -1: adaptive, 0..4: forced
int png_encode_bytes(int n, int h, int w, int c, size_t* out_stride, size_t* workspace_bytes);
int launch_png_encode_u8(const uint8_t* src, int n, int h, int w, int c, int filter, uint8_t* out, size_t out_stride, int32_t* lengths, void* workspace,
                         size_t workspace_bytes, hipStream_t s);
// png_decode.hip: PNG input files, pixel for pixel Pillow's (the rules: png_inflate.h, tests/png_decode_ref.py); offsets: HOST array [n + 1]
int png_decode_bytes(int n, int h, int w, int c_file, size_t max_stream_bytes, size_t* workspace_bytes);
int launch_png_decode_u8(const uint8_t* streams, size_t streams_bytes, const uint64_t* offsets, int n, int h, int w, int c_file, int c_out, uint8_t* out,
                         int32_t* record, void* workspace, size_t workspace_bytes, hipStream_t s);

// palette.hip: the palette page's recolouring, tone step and error diffusion (the rules: top of palette.hip, tests/palette_ref.py);
// the launchers refuse everything themselves
int launch_palette_map_u8(const uint8_t* src, int n, int h, int w, const uint8_t* palette, int K, int metric, const uint8_t* lut, int grey, uint8_t* out,
                          uint8_t* index, hipStream_t s);
int launch_tone_u8(const uint8_t* src, int n, int h, int w, const uint8_t* lut, int grey, uint8_t* out, hipStream_t s);
int palette_dither_bytes(int n, int h, int w, size_t* workspace_bytes);
int launch_palette_dither_u8(const uint8_t* src, int n, int h, int w, const uint8_t* palette, int K, const uint8_t* lut, int grey, uint8_t* out, uint8_t* index,
                             void* workspace, size_t workspace_bytes, hipStream_t s);

// gif.hip: an animated GIF's frame records from palette index planes (the rules: top of gif.hip, tests/gif_ref.py); the launcher refuses
// everything itself
int gif_encode_bytes(int n, int h, int w, int K, size_t* out_stride, size_t* workspace_bytes);
int launch_gif_encode_u8(const uint8_t* index, int n, int h, int w, int K, int delay_cs, uint8_t* out, size_t out_stride, int32_t* lengths, void* workspace,
                         size_t workspace_bytes, hipStream_t s);

// quantize.hip: a palette of at most 256 colours chosen from the frames (the rules: top of quantize.hip, tests/quantize_ref.py); the
// launcher refuses everything itself
int quantize_palette_bytes(int n, int h, int w, int mode, size_t* workspace_bytes);
int launch_quantize_palette_u8(const uint8_t* src, int n, int h, int w, int K, int mode, uint8_t* palettes, int32_t* used, void* workspace, size_t workspace_bytes,
                               hipStream_t s);
// quantize_refine.hip: the rounds of k-means behind the cut (mode's ADAIN_QUANTIZE_REFINE bits), launched by launch_quantize_palette_u8
unsigned quantize_refine_groups(size_t palettes, size_t pixels);
void launch_quantize_refine(const uint8_t* src, size_t palettes_n, size_t pixels, unsigned groups, int K, int rounds, uint8_t* palettes, int32_t* used,
                            void* accumulators, hipStream_t s);

// metrics.hip: per-frame SSIM, MSE, L1 and PSNR of two clips (the rules: top of metrics.hip, tests/metrics_ref.py); the launchers refuse
// everything themselves
int image_metrics_u8_bytes(int n, int h, int w, int c, size_t* workspace_bytes);
int image_metrics_f32_bytes(int n, int c, int h, int w, size_t* workspace_bytes);
int launch_image_metrics_u8(const uint8_t* a, const uint8_t* b, int n, int h, int w, int c, double* out, float* ssim_map, void* workspace, size_t workspace_bytes,
                            hipStream_t s);
int launch_image_metrics_f32(const float* a, const float* b, int n, int c, int h, int w, double* out, float* ssim_map, void* workspace, size_t workspace_bytes,
                             hipStream_t s);
void ssim_window(float out[11]);
// the gradient of the float32 scores: weights [n][3] = upstream d/d{ssim, mse, l1} per frame; grad_b may be null
int image_metrics_grad_f32_bytes(int n, int c, int h, int w, int with_grad_b, size_t* workspace_bytes);
int launch_image_metrics_grad_f32(const float* a, const float* b, int n, int c, int h, int w, const double* weights, float* grad_a, float* grad_b,
                                  void* workspace, size_t workspace_bytes, hipStream_t s);

// guide_loss.hip: train.py's l1_loss of a render against its uint8 guide view, resampled on the fly, and its gradient (the rules: top of
// guide_loss.hip, tests/guide_loss_ref.py); the launchers refuse everything themselves
int guide_l1_f32_bytes(int n, int h, int w, size_t* workspace_bytes);
int launch_guide_l1_f32(const float* image, const uint8_t* guide, int n, int h, int w, int gh, int gw, double* out, float* resampled, void* workspace,
                        size_t workspace_bytes, hipStream_t s);
int launch_guide_l1_grad_f32(const float* image, const uint8_t* guide, int n, int h, int w, int gh, int gw, const double* weights, float* grad, hipStream_t s);

// coral.hip: coral(style, content) of the colour-preserving path (function.py:26-67)
size_t coral_workspace_bytes(int n, int style_n, int hs, int ws, int hc, int wc);
int launch_coral(const void* style, int style_is_u8, int style_n, int hs, int ws, const void* content, int content_is_u8, int n, int hc, int wc,
                 float* out, void* workspace, size_t ws_bytes, hipStream_t s);

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return ADAIN_ELAUNCH;
    }
    return 0;
}

}  // namespace adain
