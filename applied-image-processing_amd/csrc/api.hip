// extern "C" boundary (include/adain_hip.h) and the encoder / decoder layer schedules.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include "common.h"

namespace adain {

static thread_local char g_err[512] = "";
// launch schedule of the calling thread (adain_set_schedule): ADAIN_SCHEDULE_BATCH or ADAIN_SCHEDULE_LATENCY
static thread_local int g_schedule = ADAIN_SCHEDULE_BATCH;

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// Layer tables.  Encoder = net.vgg[:31] (reference net.py:38-69): conv0+conv1_1 folded ("first"), then
// 8 generic 3x3 convs; the ceil-mode max-pools in front of conv2_1, conv3_1, conv4_1 are fused into those
// convs' producers.  Decoder = net.decoder (net.py:6-36): 8 generic convs (the nearest-2x upsamples in front
// of the 2nd, 6th and 8th are fused into them) + the 64->3 "last" conv.
// `pool` = the layer's output feeds a max-pool: the pool is fused into this layer's EPILOGUE (only the pooled
// tensor is written), so the next conv reads it directly.  `up` = the layer reads the nearest-2x upsample of its
// source: it runs as four phase convolutions of the source (conv_wino4.hip, W4P) with their own 4 x 24 floats per
// weight pair.
struct Layer { int cin, cout, pool, up; };
static const Layer ENC[8] = {{64, 64, 1, 0},   {64, 128, 0, 0},  {128, 128, 1, 0}, {128, 256, 0, 0},
                             {256, 256, 0, 0}, {256, 256, 0, 0}, {256, 256, 1, 0}, {256, 512, 0, 0}};
static const Layer DEC[8] = {{512, 256, 0, 0}, {256, 256, 0, 1}, {256, 256, 0, 0}, {256, 256, 0, 0},
                             {256, 128, 0, 0}, {128, 128, 0, 1}, {128, 64, 0, 0},  {64, 64, 0, 1}};

constexpr size_t FIRST_W = 2 * 14 * 64, FIRST_B = 64, LAST_W = 8 * 64 * 4, LAST_B = 3;

// The generic 3x3 layers run - and the library only contains - the Winograd F(4,3) x F(2,3) kernels (csrc/conv_wino4.hip).  The direct
// implicit GEMM and the F(2x2,3x3) families of rounds 1-2 were A/B baselines until round 6 and are retired (git history;
// docs/HISTORY.md has their numbers).
static size_t form_floats(const Layer& l) { return (size_t)l.cin * l.cout * 24 * (l.up ? 4 : 1); }

// packed layout: [first w][first b] (encoder) then per generic layer [w in the form the schedules launch][b], then [last w][last b]
// (decoder), every block 256-B aligned: 75 MB for the two networks in the F(4,3) x F(2,3) form (only that form is packed and kept).
struct Offsets { size_t w[8], b[8], first_b, last_w, last_b, total; };      // floats
static Offsets offsets(const Layer* L) {
    Offsets f{};
    Carve c;
    auto floats = [&c](size_t n) { return c.take(n * sizeof(float)) / sizeof(float); };
    if (L == ENC) {
        floats(FIRST_W);            // at 0
        f.first_b = floats(FIRST_B);
    }
    for (int i = 0; i < 8; ++i) {
        f.w[i] = floats(form_floats(L[i]));
        f.b[i] = floats(L[i].cout);
    }
    if (L == DEC) {
        f.last_w = floats(LAST_W);
        f.last_b = floats(LAST_B);
    }
    f.total = c.at / sizeof(float);
    return f;
}

// a bias into its block of a packed network; the block's padding (the decoder's last bias: 3 floats of 64) is zeroed, so that a pack
// writes every float the *_packed_floats query counts and the caller's buffer needs no preparation
// One kernel, not hipMemcpyAsync + hipMemsetAsync.  Observed, not explained: with the decoder's pack captured into a hipGraph, the
// memset of the last bias's padding (244 bytes, starting 12 bytes into a 256-byte block) zeroed on the first replay and wrote a
// repeating 16-byte pattern of stray bytes on the later ones, after other data had been uploaded in between
// (tests/test_gpu_graph_capture.py, adain_decoder_pack).  What in the runtime's memset node goes wrong is not known; the library's
// other memsets replayed correctly at the one shape each has in tests/capture_cases.py, which is all that is known about them.
__global__ void copy_bias_kernel(const float* __restrict__ src, float* __restrict__ dst, int n, int padded) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < padded) dst[i] = i < n ? src[i] : 0.0f;
}

static int copy_bias(const float* src, float* dst, int n, hipStream_t s) {
    const int padded = (int)(align256((size_t)n * sizeof(float)) / sizeof(float));
    hipLaunchKernelGGL(copy_bias_kernel, dim3((padded + 255) / 256), dim3(256), 0, s, src, dst, n, padded);
    return check_launch("copy_bias");
}

static void record(void* const* ev, int i, hipStream_t s) {
    if (ev && ev[i]) (void)hipEventRecord((hipEvent_t)ev[i], s);
}

#define RET_IF(x) do { int _r = (x); if (_r) return _r; } while (0)

// the 8 generic layers' weights (w[i], b[i]) into their blocks of a packed network
static int pack_generic(const Layer* L, const float* const* w, const float* const* b, float* packed, const Offsets& f, hipStream_t s) {
    for (int i = 0; i < 8; ++i) {
        RET_IF((L[i].up ? launch_pack_up2x_poly : launch_pack_wino4)(w[i], packed + f.w[i], L[i].cin, L[i].cout, s));
        RET_IF(copy_bias(b[i], packed + f.b[i], L[i].cout, s));
    }
    return 0;
}

}  // namespace adain

using namespace adain;

extern "C" {

int adain_abi_version(void) { return ADAIN_ABI_VERSION; }
const char* adain_last_error(void) { return g_err; }

int adain_set_schedule(int schedule) {
    if (schedule != ADAIN_SCHEDULE_BATCH && schedule != ADAIN_SCHEDULE_LATENCY) { set_error("set_schedule: unknown schedule %d", schedule); return ADAIN_EINVAL; }
    const int prev = g_schedule;
    g_schedule = schedule;
    return prev;
}
int adain_get_schedule(void) { return g_schedule; }

size_t adain_encoder_packed_floats(void) { return offsets(ENC).total; }
size_t adain_decoder_packed_floats(void) { return offsets(DEC).total; }

int adain_encoder_pack(const float* const* w, const float* const* b, float* packed, adain_stream_t stream) {
    if (!w || !b || !packed) { set_error("encoder_pack: null pointer"); return ADAIN_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const Offsets f = offsets(ENC);
    RET_IF(launch_pack_conv_first(w[0], b[0], w[1], b[1], packed, packed + f.first_b, s));
    return pack_generic(ENC, w + 2, b + 2, packed, f, s);
}

int adain_decoder_pack(const float* const* w, const float* const* b, float* packed, adain_stream_t stream) {
    if (!w || !b || !packed) { set_error("decoder_pack: null pointer"); return ADAIN_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const Offsets f = offsets(DEC);
    RET_IF(pack_generic(DEC, w, b, packed, f, s));
    RET_IF(launch_pack_conv_last(w[8], packed + f.last_w, s));
    return copy_bias(b[8], packed + f.last_b, 3, s);
}

void adain_encoded_size(int h, int w, int* hc, int* wc) {
    for (int i = 0; i < 3; ++i) { h = (h + 1) / 2; w = (w + 1) / 2; }
    if (hc) *hc = h;
    if (wc) *wc = w;
}

// ---- one network over one call: the plan every size, buffer and launch of its schedules is read from ----------------------------------
// Per generic layer l: the source size (Hs, Ws), the conv size (H, W: twice the source for an up layer), the stored output size (Ho, Wo:
// halved, ceil mode, where the layer pools), the output floats per image, and the ping-pong buffer the layer writes - the one its input
// is not in.  The encoder's input is conv_first's 64-channel output in buffer A and its conv4_1 (layer 7) writes the caller's feature
// tensor; the decoder's input is the caller's feature tensor.  The workspace is [A][B][slabs]: A and B hold the maxima over the layers
// that write them (ceil-mode pooling makes odd sizes non-monotonic), the slabs take the partial sums of the layers that
// ADAIN_SCHEDULE_LATENCY would split along cin (conv_wino4.hip: only launches with fewer tiles than compute units - single frames of the
// 256 class; at most 8 MB).  The slabs are always part of the workspace, whatever the calling thread's schedule is when it asks for the size.
constexpr int BUF_A = 0, BUF_B = 1, CALLER = -1;     // NetPlan::in_buf, NetPlan::buf: a ping-pong buffer or a tensor of the caller
struct NetPlan {
    const Layer* L;
    int n;
    int Hs[8], Ws[8], H[8], W[8], Ho[8], Wo[8];
    size_t out_img[8];                                 // output floats per image
    int buf[8];
    int in_buf;                                        // where layer 0's input is
    size_t o_buf[2], o_slab, total;                    // the workspace [A][B][slabs]: offsets and size in bytes
    size_t slab_floats;                                // the slab block's floats, rounded up to its 256 bytes; 0: no layer would be split
    // the call's tensors (place()): the two buffers, the slab workspace, the caller's input / output tensor
    float* bufs[2];
    float* slab;
    const float* in;
    float* out;
};
static NetPlan net_plan(const Layer* L, int n, int h, int w) {
    NetPlan p{};
    p.L = L;
    p.n = n;
    p.in_buf = L == ENC ? BUF_A : CALLER;
    size_t mx[2] = {0, 0}, slab = 0;
    if (p.in_buf == BUF_A) mx[BUF_A] = (size_t)n * h * w * L[0].cin;
    int in_buf = p.in_buf;
    for (int l = 0; l < 8; ++l) {
        p.Hs[l] = h; p.Ws[l] = w;
        p.H[l] = L[l].up ? 2 * h : h; p.W[l] = L[l].up ? 2 * w : w;
        p.Ho[l] = L[l].pool ? (p.H[l] + 1) / 2 : p.H[l]; p.Wo[l] = L[l].pool ? (p.W[l] + 1) / 2 : p.W[l];
        p.out_img[l] = (size_t)p.Ho[l] * p.Wo[l] * L[l].cout;
        p.buf[l] = (L == ENC && l == 7) ? CALLER : (in_buf == BUF_A ? BUF_B : BUF_A);
        if (p.buf[l] >= 0 && (size_t)n * p.out_img[l] > mx[p.buf[l]]) mx[p.buf[l]] = (size_t)n * p.out_img[l];
        const size_t f = wino4_split_floats(n, p.H[l], p.W[l], L[l].cin, L[l].cout);
        if (f > slab) slab = f;
        in_buf = p.buf[l];
        h = p.Ho[l]; w = p.Wo[l];
    }
    Carve c;
    p.o_buf[BUF_A] = c.take(mx[BUF_A] * sizeof(float));
    p.o_buf[BUF_B] = c.take(mx[BUF_B] * sizeof(float));
    p.o_slab = c.take(slab * sizeof(float));      // the slabs themselves are the kernel's own layout (wino4_split_floats), left alone
    p.total = c.at;
    p.slab_floats = (p.total - p.o_slab) / sizeof(float);
    return p;
}
// the plan's workspace is at ws; in / out: the caller's tensors the network reads / writes in place of a buffer
static void place(NetPlan& p, char* ws, const float* in, float* out) {
    p.bufs[BUF_A] = (float*)(ws + p.o_buf[BUF_A]);
    p.bufs[BUF_B] = (float*)(ws + p.o_buf[BUF_B]);
    p.slab = (float*)(ws + p.o_slab);
    p.in = in;
    p.out = out;
}
static SplitWs split_ws(const NetPlan& p) {
    return (g_schedule == ADAIN_SCHEDULE_LATENCY && p.slab_floats) ? SplitWs{p.slab, p.slab_floats} : SplitWs{nullptr, 0};
}

// floats per image of layer l's source
static size_t src_img(const NetPlan& p, int l) { return (size_t)p.Hs[l] * p.Ws[l] * p.L[l].cin; }
// layer l of a placed plan over images [i0, i0 + k): source and output at i0 x their per-image sizes
static ConvArgs layer_args(const NetPlan& p, int l, int i0, int k, const float* packed, const Offsets& f) {
    const Layer& L = p.L[l];
    const int src = l ? p.buf[l - 1] : p.in_buf;
    ConvArgs a{};
    a.cin = L.cin; a.cout = L.cout; a.relu = 1; a.pool_out = L.pool;
    a.bias = packed + f.b[l]; a.wpk = packed + f.w[l];
    a.in = (src < 0 ? p.in : p.bufs[src]) + (size_t)i0 * src_img(p, l);
    a.out = (p.buf[l] < 0 ? p.out : p.bufs[p.buf[l]]) + (size_t)i0 * p.out_img[l];
    a.n = k; a.H = p.H[l]; a.W = p.W[l]; a.Hs = p.Hs[l]; a.Ws = p.Ws[l];
    return a;
}
// layers [l0, l1) over images [i0, i0 + k); ev[l] (if given) is recorded after layer l.  Up layers run in their polyphase form, which
// is never split along cin.
static int run_layers(const NetPlan& p, int l0, int l1, int i0, int k, const float* packed, const Offsets& f, SplitWs split, void* const* ev,
                      hipStream_t s) {
    for (int l = l0; l < l1; ++l) {
        const ConvArgs a = layer_args(p, l, i0, k, packed, f);
        RET_IF(p.L[l].up ? launch_conv3x3_up2x_poly(a, s) : launch_conv3x3_wino4(a, SRC_DIRECT, s, split));
        record(ev, l, s);
    }
    return 0;
}

size_t adain_encode_workspace_bytes(int n, int h, int w) {
    if (n < 1 || h < 1 || w < 1) return 0;
    return net_plan(ENC, n, h, w).total;
}

size_t adain_encode_multi_workspace_bytes(int count, const int* n, const int* h, const int* w) {
    if (count < 1 || count > MAX_CONV_SEGS || !n || !h || !w) return 0;
    size_t total = 0;
    for (int i = 0; i < count; ++i) total += adain_encode_workspace_bytes(n[i], h[i], w[i]);
    return total;
}

size_t adain_decode_workspace_bytes(int n, int hc, int wc) {
    if (n < 1 || hc < 1 || wc < 1) return 0;
    return net_plan(DEC, n, hc, wc).total;
}

// ---- batches of WIDE frames: which layers run frame by frame -----------------------------------------------------------------------
// Measured (profiles/r04_batching_per_layer.md, tools/probes/frame_major_ab.sh): for 1080p and 1200 x 1600 frames a launch over a
// whole batch costs the mid-network layers a few per cent against one launch per frame in frame-major order, while the small
// relu4-level layers GAIN from the batch (one 1080p frame is 2.1 rounds of work for the resident workgroups in dec1, run in 3).
// Same-box A/B of the two schedules at batch 2 / 4: W = 1920 +0.5 / +1.7 %, W = 1600 +0.4 / +1.3 %, W = 1536 +0.3 %, but W = 1408
// -1.2 / -0.4 %, W = 1280 -1.0 / -1.6 %, W = 960 -1.8 %: the sign follows the frame's WIDTH - a tile row of the 128-channel half-size
// layers (10 halo rows x W/2 pixels x 512 B) outgrows an XCD's 4 MB L2 at W = 1638 - and below it a batch only helps (fewer launch
// ramps, fuller last rounds).  So a batch of frames at least BIG_FRAME_WIDTH wide runs its BIG layers - one frame alone is worth at
// least BIG_LAYER_ROUNDS rounds of the persistent grid - frame by frame (everything from the image down to the last big layer for
// frame 0, then for frame 1, ...) and only the layers behind them once over all frames; narrower frames run every layer over the
// batch, as they always did.  Results do not depend on the split.
constexpr double BIG_LAYER_ROUNDS = 6.0;
constexpr int BIG_FRAME_WIDTH = 1600;
static bool big_layer(const NetPlan& p, int l) { return wino4_rounds_per_image(p.H[l], p.W[l], p.L[l].cout) >= BIG_LAYER_ROUNDS; }

// encoder: number of leading generic layers (0..7) run frame by frame = index after the LAST big layer.  conv4_1 (layer 7) is never
// part of the prefix: it writes the caller's feature tensors, not the ping-pong buffers the frame-major pass works in, so it always
// runs over the whole batch in the layer-major loop behind (a 1440 x 2560 frame's conv4_1 is 7.2 rounds and would count as big).
static int enc_frame_major_layers(const NetPlan& p) {
    if (p.n < 2 || p.Ws[0] < BIG_FRAME_WIDTH) return 0;
    int k = 0;
    for (int l = 0; l < 7; ++l)
        if (big_layer(p, l)) k = l + 1;
    return k;
}
// decoder: number of leading layers (0..8) run over the whole batch = index of the FIRST big layer (8: none is big)
static int dec_batched_layers(const NetPlan& p) {
    if (p.n < 2 || p.W[7] < BIG_FRAME_WIDTH) return 8;           // W[7]: the width of the decoded frames
    for (int l = 0; l < 8; ++l)
        if (big_layer(p, l)) return l;
    return 8;
}

// The frame-by-frame passes share the batched schedule's two ping-pong buffers (image i's tensor of a layer sits at i x that layer's
// per-image size, where the batched layers expect it).  A pass runs layers [first, last) for one image after the other (first == -1:
// conv_first's output, the encoder's input, too), and tensor `keep` of every image must survive the passes of the images behind it:
// the encoder keeps the LAST frame-major tensor of the images processed earlier, the decoder - images processed LAST to FIRST - the
// batched layers' output of the images still waiting.  When image j runs, those tensors occupy [0, j x keep's size) of keep's buffer
// and image j writes tensor t at j x t's size: safe iff every tensor of the pass in that buffer is at least as large per image (j
// cancels).  With VGG's sizes it always is (later tensors of the same buffer are larger and start further out); this replays the
// offsets and says so for the case at hand - if not, every layer runs over the whole batch.
static bool frame_pass_is_safe(const NetPlan& p, int first, int last, int keep) {
    const size_t kept = p.out_img[keep];
    if (first < 0 && p.in_buf == p.buf[keep] && src_img(p, 0) < kept) return false;
    for (int l = first < 0 ? 0 : first; l < last; ++l)
        if (p.buf[l] == p.buf[keep] && p.out_img[l] < kept) return false;
    return true;
}

// images[i]: NCHW float, or (u8 != 0) HWC uint8 converted as ToTensor does inside the first layer's kernel
static int encode_impl(int count, const void* const* images, int u8, float* const* feats, const int* n, const int* h, const int* w,
                       const float* packed, void* workspace, size_t ws_bytes, void* const* ev, adain_stream_t stream) {
    if (count < 1 || count > MAX_CONV_SEGS) { set_error("encode: 1..%d image batches per call, got %d", MAX_CONV_SEGS, count); return ADAIN_EINVAL; }
    if (!images || !feats || !n || !h || !w || !packed || !workspace) { set_error("encode: null pointer"); return ADAIN_EINVAL; }
    for (int i = 0; i < count; ++i) {
        if (!images[i] || !feats[i]) { set_error("encode: null pointer"); return ADAIN_EINVAL; }
        if (n[i] < 1 || h[i] < 9 || w[i] < 9) {
            // relu4_1 must be at least 2x2 for the reflection pad in front of conv4_1 (torch raises there too)
            set_error("encode: image %dx%d too small (needs h, w >= 9)", h[i], w[i]);
            return ADAIN_EINVAL;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    const Offsets f = offsets(ENC);
    NetPlan p[MAX_CONV_SEGS];
    SplitWs split[MAX_CONV_SEGS];
    size_t need = 0;                // the batches' workspaces, one behind the other
    for (int i = 0; i < count; ++i) {
        p[i] = net_plan(ENC, n[i], h[i], w[i]);
        place(p[i], (char*)workspace + need, nullptr, feats[i]);
        need += p[i].total;
        split[i] = split_ws(p[i]);
    }
    RET_IF(check_workspace("encode", workspace, ws_bytes, need, 1));
    record(ev, 0, s);
    // a batch of large frames (one tensor pair, no per-layer events wanted): conv_first and its big layers frame by frame, see above,
    // leaving every image's tensors where the layer-major loop behind expects them
    int frame_major = (count == 1 && !ev) ? enc_frame_major_layers(p[0]) : 0;
    if (frame_major && !frame_pass_is_safe(p[0], -1, frame_major, frame_major - 1)) frame_major = 0;
    if (frame_major) {
        const size_t img_bytes = (size_t)h[0] * w[0] * 3 * (u8 ? 1 : 4);
        for (int j = 0; j < n[0]; ++j) {
            RET_IF(launch_conv_first((const char*)images[0] + j * img_bytes, u8, p[0].bufs[BUF_A] + j * src_img(p[0], 0), packed, packed + f.first_b,
                                     1, h[0], w[0], s));
            RET_IF(run_layers(p[0], 0, frame_major, j, 1, packed, f, SplitWs{nullptr, 0}, nullptr, s));
        }
    } else {
        for (int i = 0; i < count; ++i)
            RET_IF(launch_conv_first(images[i], u8, p[i].bufs[BUF_A], packed, packed + f.first_b, n[i], h[i], w[i], s));
    }
    record(ev, 1, s);
    for (int l = frame_major; l < 8; ++l) {
        // one launch for every batch: the persistent kernel's tile list runs over all of them (csrc/conv_wino4.hip, SEGMENTS)
        ConvSeg segs[MAX_CONV_SEGS];
        for (int i = 0; i < count; ++i) {
            const ConvArgs a = layer_args(p[i], l, 0, n[i], packed, f);
            segs[i] = ConvSeg{a.in, a.out, a.n, a.H, a.W, a.Hs, a.Ws, 0, 0, 0};
        }
        RET_IF(launch_conv3x3_wino4_multi(layer_args(p[0], l, 0, n[0], packed, f), segs, count, SRC_DIRECT, s, split));
        record(ev, l + 2, s);
    }
    return 0;
}

int adain_encode_multi(int count, const float* const* images, float* const* feats, const int* n, const int* h, const int* w,
                       const float* packed, void* workspace, size_t ws_bytes, void* const* ev, adain_stream_t stream) {
    return encode_impl(count, (const void* const*)images, 0, feats, n, h, w, packed, workspace, ws_bytes, ev, stream);
}

int adain_encode(const float* image, float* feat, const float* packed, void* workspace, size_t ws_bytes, int n, int h,
                 int w, void* const* ev, adain_stream_t stream) {
    if (!image || !feat) { set_error("encode: null pointer"); return ADAIN_EINVAL; }
    const void* img = image;
    return encode_impl(1, &img, 0, &feat, &n, &h, &w, packed, workspace, ws_bytes, ev, stream);
}

int adain_encode_u8(const uint8_t* image, float* feat, const float* packed, void* workspace, size_t ws_bytes, int n, int h,
                    int w, void* const* ev, adain_stream_t stream) {
    if (!image || !feat) { set_error("encode: null pointer"); return ADAIN_EINVAL; }
    const void* img = image;
    return encode_impl(1, &img, 1, &feat, &n, &h, &w, packed, workspace, ws_bytes, ev, stream);
}

int adain_encode_relu1_1(const void* image, int is_u8, float* relu1_1, const float* packed, int n, int h, int w, adain_stream_t stream) {
    if (!image || !relu1_1 || !packed) { set_error("encode_relu1_1: null pointer"); return ADAIN_EINVAL; }
    if (n < 1 || h < 2 || w < 2) { set_error("encode_relu1_1: image %dx%d too small (the reflection pad needs h, w >= 2)", h, w); return ADAIN_EINVAL; }
    const Offsets f = offsets(ENC);
    return launch_conv_first(image, is_u8 ? 1 : 0, relu1_1, packed, packed + f.first_b, n, h, w, (hipStream_t)stream);
}

// image_u8 != nullptr: the last layer writes save_image's uint8 HWC frames itself (adain_stylize_u8 without a mask: the bytes of
// adain_decode + adain_quantize_u8, one launch and the float image's round trip through HBM less); image is then unused
static int decode_impl(const float* feat, float* image, uint8_t* image_u8, const float* packed, void* workspace, size_t ws_bytes, int n, int hc,
                       int wc, void* const* ev, adain_stream_t stream) {
    if (!feat || (!image && !image_u8) || !packed || !workspace) { set_error("decode: null pointer"); return ADAIN_EINVAL; }
    if (n < 1 || hc < 2 || wc < 2) { set_error("decode: feature map %dx%d too small (needs >= 2x2)", hc, wc); return ADAIN_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const Offsets f = offsets(DEC);
    NetPlan p = net_plan(DEC, n, hc, wc);
    RET_IF(check_workspace("decode", workspace, ws_bytes, p.total, 1));
    place(p, (char*)workspace, feat, nullptr);
    record(ev, 0, s);
    // a batch of large frames: the leading small layers over the whole batch, then everything from the first big layer to the
    // image frame by frame, images last to first (see enc_frame_major_layers, frame_pass_is_safe)
    int batched = !ev ? dec_batched_layers(p) : 8;
    if (batched > 0 && batched < 8 && !frame_pass_is_safe(p, batched, 8, batched - 1)) batched = 8;
    RET_IF(run_layers(p, 0, batched, 0, n, packed, f, split_ws(p), ev ? ev + 1 : nullptr, s));
    const float* last = p.bufs[p.buf[7]];
    const int H = p.H[7], W = p.W[7];
    if (batched == 8) {
        RET_IF(launch_conv_last(last, image, packed + f.last_w, packed + f.last_b, n, H, W, s, image_u8));
        record(ev, 9, s);
        return 0;
    }
    for (int img = n - 1; img >= 0; --img) {
        RET_IF(run_layers(p, batched, 8, img, 1, packed, f, SplitWs{nullptr, 0}, nullptr, s));
        RET_IF(launch_conv_last(last + (size_t)img * p.out_img[7], image ? image + (size_t)img * 3 * H * W : nullptr, packed + f.last_w,
                                packed + f.last_b, 1, H, W, s, image_u8 ? image_u8 + (size_t)img * 3 * H * W : nullptr));
    }
    return 0;
}

int adain_decode(const float* feat, float* image, const float* packed, void* workspace, size_t ws_bytes, int n, int hc,
                 int wc, void* const* ev, adain_stream_t stream) {
    if (!image) { set_error("decode: null pointer"); return ADAIN_EINVAL; }
    return decode_impl(feat, image, nullptr, packed, workspace, ws_bytes, n, hc, wc, ev, stream);
}

size_t adain_mean_std_workspace_bytes(int nhwc, int n, int c, int hw) { return mean_std_workspace_bytes(nhwc, n, c, hw); }

int adain_mean_std(const float* feat, int nhwc, int n, int c, int hw, float eps, float* mean, float* std_out, void* workspace,
                   size_t ws_bytes, adain_stream_t stream) {
    if (!feat || !mean || !std_out) { set_error("mean_std: null pointer"); return ADAIN_EINVAL; }
    return launch_mean_std(feat, nhwc, n, c, hw, eps, mean, std_out, workspace, ws_bytes, (hipStream_t)stream);
}

// s_mean / s_std [style_n][c] of the single-style entries: one row for every frame, or one row per frame
static int blend_single(const float* x, int nhwc, int n, int c, int hw, const float* c_mean, const float* c_std, const float* s_mean,
                        const float* s_std, int style_n, const BlendTerm& blend, float* out, adain_stream_t stream) {
    if (style_n != 1 && style_n != n) { set_error("adain_blend: style batch %d must be 1 or %d", style_n, n); return ADAIN_EINVAL; }
    return launch_adain_blend(x, nhwc, n, c, hw, c_mean, c_std, StyleTerm{s_mean, s_std, 1, style_n == n, nullptr, 1, 1}, blend, out, (hipStream_t)stream);
}

int adain_blend_alpha(const float* x, int nhwc, int n, int c, int hw, const float* c_mean, const float* c_std,
                      const float* s_mean, const float* s_std, int style_n, float alpha, float one_minus_alpha, float* out,
                      adain_stream_t stream) {
    if (!x || !c_mean || !c_std || !s_mean || !s_std || !out) { set_error("blend_alpha: null pointer"); return ADAIN_EINVAL; }
    return blend_single(x, nhwc, n, c, hw, c_mean, c_std, s_mean, s_std, style_n, BlendTerm{alpha, one_minus_alpha, nullptr, 1}, out, stream);
}

int adain_blend_pmap(const float* x, int nhwc, int n, int c, int hw, const float* c_mean, const float* c_std,
                     const float* s_mean, const float* s_std, int style_n, const float* pmap, int pmap_n, float* out,
                     adain_stream_t stream) {
    if (!x || !c_mean || !c_std || !s_mean || !s_std || !out || !pmap) { set_error("blend_pmap: null pointer"); return ADAIN_EINVAL; }
    return blend_single(x, nhwc, n, c, hw, c_mean, c_std, s_mean, s_std, style_n, BlendTerm{0.f, 0.f, pmap, pmap_n}, out, stream);
}

int adain_blend_mix(const float* x, int nhwc, int n, int c, int hw, const float* c_mean, const float* c_std, const float* s_mean,
                    const float* s_std, int k, const float* weights, int weights_n, int weights_hw, float alpha, float one_minus_alpha,
                    const float* pmap, int pmap_n, float* out, adain_stream_t stream) {
    if (!x || !c_mean || !c_std || !s_mean || !s_std || !weights || !out) { set_error("blend_mix: null pointer"); return ADAIN_EINVAL; }
    return launch_adain_blend(x, nhwc, n, c, hw, c_mean, c_std, StyleTerm{s_mean, s_std, k, 0, weights, weights_n, weights_hw},
                              BlendTerm{alpha, one_minus_alpha, pmap, pmap_n}, out, (hipStream_t)stream);
}

size_t adain_strength_map_workspace_bytes(int hc, int wc) { return strength_map_workspace_bytes(hc, wc); }

int adain_strength_map(const float* depth, int h0, int w0, int hc, int wc, float offset, float prominence, float* pmap,
                       void* workspace, size_t ws_bytes, adain_stream_t stream) {
    if (!depth || !pmap) { set_error("strength_map: null pointer"); return ADAIN_EINVAL; }
    return launch_strength_map(depth, h0, w0, hc, wc, offset, prominence, pmap, workspace, ws_bytes, (hipStream_t)stream);
}

int adain_resize_bilinear(const float* in, float* out, int planes, int hi, int wi, int ho, int wo, adain_stream_t stream) {
    if (!in || !out) { set_error("resize_bilinear: null pointer"); return ADAIN_EINVAL; }
    return launch_resize_bilinear(in, out, planes, hi, wi, ho, wo, (hipStream_t)stream);
}
int adain_resize_nearest(const float* in, float* out, int planes, int hi, int wi, int ho, int wo, adain_stream_t stream) {
    if (!in || !out) { set_error("resize_nearest: null pointer"); return ADAIN_EINVAL; }
    return launch_resize_nearest(in, out, planes, hi, wi, ho, wo, (hipStream_t)stream);
}
int adain_mask_composite(const float* content, const float* stylized, const float* mask, int mask_c, int mask_n, float* out, int n,
                         int c, int hw, adain_stream_t stream) {
    if (!content || !stylized || !mask || !out) { set_error("mask_composite: null pointer"); return ADAIN_EINVAL; }
    return launch_mask_composite(content, stylized, mask, mask_c, mask_n, out, n, c, hw, (hipStream_t)stream);
}
int adain_quantize_u8(const float* in, uint8_t* out, int n, int c, int h, int w, adain_stream_t stream) {
    if (!in || !out) { set_error("quantize_u8: null pointer"); return ADAIN_EINVAL; }
    return launch_quantize_u8(in, out, n, c, h, w, (hipStream_t)stream);
}
int adain_u8_to_f32(const uint8_t* in, float* out, int n, int c, int h, int w, adain_stream_t stream) {
    if (!in || !out) { set_error("u8_to_f32: null pointer"); return ADAIN_EINVAL; }
    return launch_u8_to_f32(in, out, n, c, h, w, (hipStream_t)stream);
}
int adain_warp_blend_u8(const uint8_t* cur, const uint8_t* prev, const float* flow, uint8_t* out, int h, int w, int c, float alpha,
                        float one_minus_alpha, adain_stream_t stream) {
    if (!cur || !prev || !flow || !out) { set_error("warp_blend_u8: null pointer"); return ADAIN_EINVAL; }
    return launch_warp_blend_u8(cur, prev, flow, out, h, w, c, alpha, one_minus_alpha, (hipStream_t)stream);
}
int adain_flow_gray_u8(const uint8_t* rgb_u8, int n, int hi, int wi, uint8_t* gray_u8, int ho, int wo, adain_stream_t stream) {
    if (!rgb_u8 || !gray_u8) { set_error("flow_gray_u8: null pointer"); return ADAIN_EINVAL; }
    return launch_flow_gray_u8(rgb_u8, n, hi, wi, gray_u8, ho, wo, (hipStream_t)stream);
}
int adain_farneback_levels(int h, int w, double pyr_scale, int levels, int* out_levels, int* sizes_wh, int* ksizes, double* sigmas) {
    return farneback_levels(h, w, pyr_scale, levels, out_levels, sizes_wh, ksizes, sigmas);
}
size_t adain_farneback_pyramid_bytes(int h, int w, double pyr_scale, int levels) { return farneback_pyramid_bytes(h, w, pyr_scale, levels); }
size_t adain_farneback_workspace_bytes(int h, int w) { return farneback_workspace_bytes(h, w); }
int adain_farneback_expand(const uint8_t* gray_u8, int h, int w, double pyr_scale, int levels, int poly_n, double poly_sigma, float* pyramid,
                           void* workspace, size_t workspace_bytes, adain_stream_t stream) {
    if (!gray_u8 || !pyramid) { set_error("farneback_expand: null pointer"); return ADAIN_EINVAL; }
    return launch_farneback_expand(gray_u8, h, w, pyr_scale, levels, poly_n, poly_sigma, pyramid, workspace, workspace_bytes,
                                   (hipStream_t)stream);
}
int adain_farneback_flow(const float* pyr_prev, const float* pyr_next, int h, int w, double pyr_scale, int levels, int winsize, int iterations,
                         int flags, float* flow_out, void* workspace, size_t workspace_bytes, adain_stream_t stream) {
    if (!pyr_prev || !pyr_next || !flow_out) { set_error("farneback_flow: null pointer"); return ADAIN_EINVAL; }
    return launch_farneback_flow(pyr_prev, pyr_next, h, w, pyr_scale, levels, winsize, iterations, flags, flow_out, workspace,
                                 workspace_bytes, (hipStream_t)stream);
}
int adain_tvl1_scales(int h, int w, const adain_tvl1_params* params, int* out_nscales, int* sizes_wh) {
    return tvl1_scales(h, w, params, out_nscales, sizes_wh);
}
size_t adain_tvl1_frame_bytes(int h, int w, const adain_tvl1_params* params) { return tvl1_frame_bytes(h, w, params); }
int adain_tvl1_prepare(const uint8_t* gray_u8, int n, int h, int w, const adain_tvl1_params* params, float* prepared,
                       adain_stream_t stream) {
    if (!gray_u8 || !prepared) { set_error("tvl1_prepare: null pointer"); return ADAIN_EINVAL; }
    return launch_tvl1_prepare(gray_u8, n, h, w, params, prepared, (hipStream_t)stream);
}
size_t adain_tvl1_workspace_bytes(int h, int w, int npairs, const adain_tvl1_params* params) {
    return tvl1_workspace_bytes(h, w, npairs, params);
}
int adain_tvl1_flow(const float* const* prev_frames, const float* const* next_frames, int npairs, int h, int w,
                    const adain_tvl1_params* params, float* flows_out, int* iters_out, void* workspace, size_t workspace_bytes,
                    adain_stream_t stream) {
    if (!prev_frames || !next_frames || !flows_out) { set_error("tvl1_flow: null pointer"); return ADAIN_EINVAL; }
    return launch_tvl1_flow(prev_frames, next_frames, npairs, h, w, params, flows_out, iters_out, workspace, workspace_bytes,
                            (hipStream_t)stream);
}
int adain_resize_area_u8(const uint8_t* in, uint8_t* out, int n, int hi, int wi, int c, int ho, int wo, adain_stream_t stream) {
    if (!in || !out) { set_error("resize_area_u8: null pointer"); return ADAIN_EINVAL; }
    return launch_resize_area_u8(in, out, n, hi, wi, c, ho, wo, (hipStream_t)stream);
}
size_t adain_resize_pil_bilinear_u8_workspace_bytes(int hi, int wi, int ho, int wo) { return resize_pil_workspace_bytes(hi, wi, ho, wo); }

int adain_resize_pil_bilinear_u8(const uint8_t* in, int pixel_bytes, int n, int hi, int wi, uint8_t* out, int ho, int wo, int crop_y0, int crop_x0,
                                 int crop_h, int crop_w, void* workspace, size_t ws_bytes, adain_stream_t stream) {
    if (!in || !out) { set_error("resize_pil_bilinear_u8: null pointer"); return ADAIN_EINVAL; }
    return launch_resize_pil_bilinear_u8(in, pixel_bytes, n, hi, wi, out, ho, wo, crop_y0, crop_x0, crop_h, crop_w, workspace, ws_bytes,
                                         (hipStream_t)stream);
}

// PIL.Image.resize for all six filters (resample_filters.hip): the table builder is host code, the launcher refuses everything itself
int adain_pil_resize_taps_bytes(int filter, int in_size, int out_size, int* ksize, size_t* bytes) {
    return pil_resize_taps_bytes(filter, in_size, out_size, ksize, bytes);
}
int adain_pil_resize_taps(int filter, int in_size, int out_size, int32_t* bounds_host, int32_t* taps_host) {
    return pil_resize_taps(filter, in_size, out_size, bounds_host, taps_host);
}
int adain_resize_pil_u8_bytes(int n, int hi, int wi, int ho, int wo, int channels, int filter, int crop_y0, int crop_x0, int crop_h, int crop_w,
                              size_t* workspace_bytes) {
    return resize_pil_u8_bytes(n, hi, wi, ho, wo, channels, filter, crop_y0, crop_x0, crop_h, crop_w, workspace_bytes);
}
int adain_resize_pil_u8(const uint8_t* src, int pixel_bytes, int n, int hi, int wi, uint8_t* dst, int ho, int wo, int filter, const int32_t* x_bounds,
                        const int32_t* x_taps, int x_ksize, const int32_t* y_bounds, const int32_t* y_taps, int y_ksize, int crop_y0, int crop_x0, int crop_h,
                        int crop_w, void* workspace, size_t workspace_bytes, adain_stream_t stream) {
    return launch_resize_pil_u8(src, pixel_bytes, n, hi, wi, dst, ho, wo, filter, x_bounds, x_taps, x_ksize, y_bounds, y_taps, y_ksize, crop_y0, crop_x0,
                                crop_h, crop_w, workspace, workspace_bytes, (hipStream_t)stream);
}

int adain_jpeg_encode_opt_u8_bytes(int n, int h, int w, int c, int sampling, int optimize, size_t* out_stride, size_t* workspace_bytes) {
    return jpeg_encode_bytes("jpeg_encode_opt_u8", n, h, w, c, sampling, optimize, out_stride, workspace_bytes) ? ADAIN_EINVAL : ADAIN_OK;
}
static int jpeg_encode(const char* who, const uint8_t* src, int n, int h, int w, int c, int quality, int sampling, int optimize, uint8_t* out, size_t out_stride,
                       int32_t* lengths, void* workspace, size_t workspace_bytes, adain_stream_t stream) {
    if (!src || !out || !lengths || !workspace) { set_error("%s: null pointer", who); return ADAIN_EINVAL; }
    if (jpeg_encode_bytes(who, n, h, w, c, sampling, optimize, nullptr, nullptr)) return ADAIN_EINVAL;
    return launch_jpeg_encode_u8(who, src, n, h, w, c, quality, sampling, optimize, out, out_stride, lengths, workspace, workspace_bytes, (hipStream_t)stream);
}
int adain_jpeg_encode_opt_u8(const uint8_t* src, int n, int h, int w, int c, int quality, int sampling, int optimize, uint8_t* out, size_t out_stride,
                             int32_t* lengths, void* workspace, size_t workspace_bytes, adain_stream_t stream) {
    return jpeg_encode("jpeg_encode_opt_u8", src, n, h, w, c, quality, sampling, optimize, out, out_stride, lengths, workspace, workspace_bytes, stream);
}
// the entry from before the options: the one above at 4:2:0 with Annex K's tables
int adain_jpeg_encode_u8_bytes(int n, int h, int w, int c, size_t* out_stride, size_t* workspace_bytes) {
    return jpeg_encode_bytes("jpeg_encode_u8", n, h, w, c, 2, 0, out_stride, workspace_bytes) ? ADAIN_EINVAL : ADAIN_OK;
}
int adain_jpeg_encode_u8(const uint8_t* src, int n, int h, int w, int c, int quality, uint8_t* out, size_t out_stride, int32_t* lengths, void* workspace,
                         size_t workspace_bytes, adain_stream_t stream) {
    return jpeg_encode("jpeg_encode_u8", src, n, h, w, c, quality, 2, 0, out, out_stride, lengths, workspace, workspace_bytes, stream);
}
// Pillow's progressive=True: the same coefficients in libjpeg's simple progression, every scan under its own optimal table
int adain_jpeg_encode_progressive_u8_bytes(int n, int h, int w, int c, int sampling, size_t* out_stride, size_t* workspace_bytes) {
    return jpeg_encode_progressive_bytes(n, h, w, c, sampling, out_stride, workspace_bytes) ? ADAIN_EINVAL : ADAIN_OK;
}
int adain_jpeg_encode_progressive_u8(const uint8_t* src, int n, int h, int w, int c, int quality, int sampling, uint8_t* out, size_t out_stride, int32_t* lengths,
                                     void* workspace, size_t workspace_bytes, adain_stream_t stream) {
    if (!src || !out || !lengths || !workspace) { set_error("jpeg_encode_progressive_u8: null pointer"); return ADAIN_EINVAL; }
    if (jpeg_encode_progressive_bytes(n, h, w, c, sampling, nullptr, nullptr)) return ADAIN_EINVAL;
    return launch_jpeg_encode_progressive_u8(src, n, h, w, c, quality, sampling, out, out_stride, lengths, workspace, workspace_bytes, (hipStream_t)stream);
}

// .png outputs (test.py:243-244, video/utils.py:292-296, train.py:104-114): the launcher refuses everything itself
int adain_png_encode_u8_bytes(int n, int h, int w, int c, size_t* out_stride, size_t* workspace_bytes) {
    return png_encode_bytes(n, h, w, c, out_stride, workspace_bytes) ? ADAIN_EINVAL : ADAIN_OK;
}
int adain_png_encode_u8(const uint8_t* src, int n, int h, int w, int c, int filter, uint8_t* out, size_t out_stride, int32_t* lengths, void* workspace,
                        size_t workspace_bytes, adain_stream_t stream) {
    return launch_png_encode_u8(src, n, h, w, c, filter, out, out_stride, lengths, workspace, workspace_bytes, (hipStream_t)stream);
}

// .png inputs (train.py:86-115, test.py's content image, video/utils.py's frames): the launcher refuses everything itself
int adain_png_decode_u8_bytes(int n, int h, int w, int c_file, size_t max_stream_bytes, size_t* workspace_bytes) {
    return png_decode_bytes(n, h, w, c_file, max_stream_bytes, workspace_bytes) ? ADAIN_EINVAL : ADAIN_OK;
}
int adain_png_decode_u8(const uint8_t* streams, size_t streams_bytes, const uint64_t* offsets, int n, int h, int w, int c_file, int c_out, uint8_t* out,
                        int32_t* record, void* workspace, size_t workspace_bytes, adain_stream_t stream) {
    return launch_png_decode_u8(streams, streams_bytes, offsets, n, h, w, c_file, c_out, out, record, workspace, workspace_bytes, (hipStream_t)stream);
}

// the palette page (gui/second_page.py, _convert_image): the launchers refuse everything themselves
int adain_palette_map_u8(const uint8_t* src, int n, int h, int w, const uint8_t* palette, int K, int metric, const uint8_t* lut, int grey, uint8_t* out,
                         uint8_t* index, adain_stream_t stream) {
    return launch_palette_map_u8(src, n, h, w, palette, K, metric, lut, grey, out, index, (hipStream_t)stream);
}
int adain_tone_u8(const uint8_t* src, int n, int h, int w, const uint8_t* lut, int grey, uint8_t* out, adain_stream_t stream) {
    return launch_tone_u8(src, n, h, w, lut, grey, out, (hipStream_t)stream);
}
int adain_palette_dither_u8_bytes(int n, int h, int w, size_t* workspace_bytes) {
    return palette_dither_bytes(n, h, w, workspace_bytes) ? ADAIN_EINVAL : ADAIN_OK;
}
int adain_palette_dither_u8(const uint8_t* src, int n, int h, int w, const uint8_t* palette, int K, const uint8_t* lut, int grey, uint8_t* out, uint8_t* index,
                            void* workspace, size_t workspace_bytes, adain_stream_t stream) {
    return launch_palette_dither_u8(src, n, h, w, palette, K, lut, grey, out, index, workspace, workspace_bytes, (hipStream_t)stream);
}

// animated GIF clips (Style_3DGS/render.py:29-33; video/utils.py:374-392 writes a cv2 video instead): the launcher refuses everything itself
int adain_gif_encode_u8_bytes(int n, int h, int w, int K, size_t* out_stride, size_t* workspace_bytes) {
    return gif_encode_bytes(n, h, w, K, out_stride, workspace_bytes) ? ADAIN_EINVAL : ADAIN_OK;
}
int adain_gif_encode_u8(const uint8_t* index, int n, int h, int w, int K, int delay_cs, uint8_t* out, size_t out_stride, int32_t* lengths, void* workspace,
                        size_t workspace_bytes, adain_stream_t stream) {
    return launch_gif_encode_u8(index, n, h, w, K, delay_cs, out, out_stride, lengths, workspace, workspace_bytes, (hipStream_t)stream);
}

// the palette of a full-colour clip, chosen from its frames (what Pillow's quantize does for create_gif): the launcher refuses everything itself
int adain_quantize_palette_u8_bytes(int n, int h, int w, int mode, size_t* workspace_bytes) {
    return quantize_palette_bytes(n, h, w, mode, workspace_bytes) ? ADAIN_EINVAL : ADAIN_OK;
}
int adain_quantize_palette_u8(const uint8_t* src, int n, int h, int w, int K, int mode, uint8_t* palettes, int32_t* used, void* workspace, size_t workspace_bytes,
                              adain_stream_t stream) {
    return launch_quantize_palette_u8(src, n, h, w, K, mode, palettes, used, workspace, workspace_bytes, (hipStream_t)stream);
}

// the scores of Style_3DGS/metrics.py (utils/loss_utils.py ssim, utils/image_utils.py psnr) per frame: the launchers refuse everything themselves
int adain_image_metrics_u8_bytes(int n, int h, int w, int c, size_t* workspace_bytes) {
    return image_metrics_u8_bytes(n, h, w, c, workspace_bytes) ? ADAIN_EINVAL : ADAIN_OK;
}
int adain_image_metrics_u8(const uint8_t* a, const uint8_t* b, int n, int h, int w, int c, double* out, float* ssim_map, void* workspace, size_t workspace_bytes,
                           adain_stream_t stream) {
    return launch_image_metrics_u8(a, b, n, h, w, c, out, ssim_map, workspace, workspace_bytes, (hipStream_t)stream);
}
int adain_image_metrics_f32_bytes(int n, int c, int h, int w, size_t* workspace_bytes) {
    return image_metrics_f32_bytes(n, c, h, w, workspace_bytes) ? ADAIN_EINVAL : ADAIN_OK;
}
int adain_image_metrics_f32(const float* a, const float* b, int n, int c, int h, int w, double* out, float* ssim_map, void* workspace, size_t workspace_bytes,
                            adain_stream_t stream) {
    return launch_image_metrics_f32(a, b, n, c, h, w, out, ssim_map, workspace, workspace_bytes, (hipStream_t)stream);
}
int adain_ssim_window(float* out) {
    if (!out) { set_error("ssim_window: out is a null pointer"); return ADAIN_EINVAL; }
    ssim_window(out);
    return ADAIN_OK;
}
// their gradient for train.py's loss (utils/loss_utils.py l1_loss, ssim under autograd): the launcher refuses everything itself
int adain_image_metrics_grad_f32_bytes(int n, int c, int h, int w, int with_grad_b, size_t* workspace_bytes) {
    return image_metrics_grad_f32_bytes(n, c, h, w, with_grad_b, workspace_bytes) ? ADAIN_EINVAL : ADAIN_OK;
}
int adain_image_metrics_grad_f32(const float* a, const float* b, int n, int c, int h, int w, const double* weights, float* grad_a, float* grad_b, void* workspace,
                                 size_t workspace_bytes, adain_stream_t stream) {
    return launch_image_metrics_grad_f32(a, b, n, c, h, w, weights, grad_a, grad_b, workspace, workspace_bytes, (hipStream_t)stream);
}

// train.py's guide-view loss (Style_3DGS/train.py:208-221) and its gradient: the launchers refuse everything themselves
int adain_guide_l1_f32_bytes(int n, int h, int w, size_t* workspace_bytes) {
    return guide_l1_f32_bytes(n, h, w, workspace_bytes) ? ADAIN_EINVAL : ADAIN_OK;
}
int adain_guide_l1_f32(const float* image, const uint8_t* guide, int n, int h, int w, int gh, int gw, double* out, float* resampled, void* workspace,
                       size_t workspace_bytes, adain_stream_t stream) {
    return launch_guide_l1_f32(image, guide, n, h, w, gh, gw, out, resampled, workspace, workspace_bytes, (hipStream_t)stream);
}
int adain_guide_l1_grad_f32(const float* image, const uint8_t* guide, int n, int h, int w, int gh, int gw, const double* weights, float* grad,
                            adain_stream_t stream) {
    return launch_guide_l1_grad_f32(image, guide, n, h, w, gh, gw, weights, grad, (hipStream_t)stream);
}

int adain_jpeg_roundtrip_u8_bytes(int n, int h, int w, int c, size_t* workspace_bytes) {
    return jpeg_roundtrip_bytes(n, h, w, c, workspace_bytes) ? ADAIN_EINVAL : ADAIN_OK;
}
int adain_jpeg_roundtrip_u8(const uint8_t* src, int n, int h, int w, int c, int quality, uint8_t* dst, void* workspace, size_t workspace_bytes,
                            adain_stream_t stream) {
    if (!src || !dst || !workspace) { set_error("jpeg_roundtrip_u8: null pointer"); return ADAIN_EINVAL; }
    if (jpeg_roundtrip_bytes(n, h, w, c, nullptr)) return ADAIN_EINVAL;       // the shape, before its product is used
    const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst, bytes = (uintptr_t)n * h * w * c;
    if (a < b + bytes && b < a + bytes) { set_error("jpeg_roundtrip_u8: dst overlaps src"); return ADAIN_EINVAL; }
    return launch_jpeg_roundtrip_u8(src, n, h, w, c, quality, dst, workspace, workspace_bytes, (hipStream_t)stream);
}

int adain_jpeg_decode_restart_u8_bytes(int n, int h, int w, int c, int sampling, int restart_interval, size_t max_segment_bytes, int chunk_bits,
                                       size_t* workspace_bytes) {
    return jpeg_decode_bytes(n, h, w, c, sampling, restart_interval, max_segment_bytes, chunk_bits, workspace_bytes) ? ADAIN_EINVAL : ADAIN_OK;
}
int adain_jpeg_decode_restart_u8(const uint8_t* files, size_t files_bytes, const uint8_t* blobs, int n, int h, int w, int c, int sampling, int restart_interval,
                                 const uint64_t* segment_offsets, const uint32_t* segment_lengths, uint8_t* dst, int32_t* record, void* workspace,
                                 size_t workspace_bytes, int chunk_bits, adain_stream_t stream) {
    if (!files || !blobs || !segment_offsets || !segment_lengths || !dst || !record || !workspace) { set_error("jpeg_decode_u8: null pointer"); return ADAIN_EINVAL; }
    return launch_jpeg_decode_u8(files, files_bytes, blobs, n, h, w, c, sampling, restart_interval, segment_offsets, segment_lengths, dst, record, workspace,
                                 workspace_bytes, chunk_bits, (hipStream_t)stream);
}
// the entries from before restart intervals: the ones above at 0
int adain_jpeg_decode_u8_bytes(int n, int h, int w, int c, int sampling, size_t max_segment_bytes, int chunk_bits, size_t* workspace_bytes) {
    return adain_jpeg_decode_restart_u8_bytes(n, h, w, c, sampling, 0, max_segment_bytes, chunk_bits, workspace_bytes);
}
int adain_jpeg_decode_u8(const uint8_t* files, size_t files_bytes, const uint8_t* blobs, int n, int h, int w, int c, int sampling,
                         const uint64_t* segment_offsets, const uint32_t* segment_lengths, uint8_t* dst, int32_t* record, void* workspace,
                         size_t workspace_bytes, int chunk_bits, adain_stream_t stream) {
    return adain_jpeg_decode_restart_u8(files, files_bytes, blobs, n, h, w, c, sampling, 0, segment_offsets, segment_lengths, dst, record, workspace, workspace_bytes,
                                        chunk_bits, stream);
}
// progressive (SOF2) files: one call per (geometry, scan script)
int adain_jpeg_decode_progressive_u8_bytes(int n, int h, int w, int c, int sampling, int nscans, size_t max_segment_bytes, int chunk_bits, size_t* workspace_bytes) {
    return jpeg_decode_progressive_bytes(n, h, w, c, sampling, nscans, max_segment_bytes, chunk_bits, workspace_bytes) ? ADAIN_EINVAL : ADAIN_OK;
}
int adain_jpeg_decode_progressive_u8(const uint8_t* files, size_t files_bytes, const uint8_t* blobs, int n, int h, int w, int c, int sampling, int nscans,
                                     const int32_t* scans, const uint64_t* segment_offsets, const uint32_t* segment_lengths, uint8_t* dst, int32_t* record,
                                     void* workspace, size_t workspace_bytes, int chunk_bits, adain_stream_t stream) {
    if (!files || !blobs || !scans || !segment_offsets || !segment_lengths || !dst || !record || !workspace) {
        set_error("jpeg_decode_progressive_u8: null pointer");
        return ADAIN_EINVAL;
    }
    return launch_jpeg_decode_progressive_u8(files, files_bytes, blobs, n, h, w, c, sampling, nscans, scans, segment_offsets, segment_lengths, dst, record,
                                             workspace, workspace_bytes, chunk_bits, (hipStream_t)stream);
}

int adain_nhwc_to_nchw(const float* in, float* out, int n, int c, int hw, adain_stream_t stream) {
    if (!in || !out) { set_error("nhwc_to_nchw: null pointer"); return ADAIN_EINVAL; }
    return launch_nhwc_to_nchw(in, out, n, c, hw, (hipStream_t)stream);
}
int adain_nchw_to_nhwc(const float* in, float* out, int n, int c, int hw, adain_stream_t stream) {
    if (!in || !out) { set_error("nchw_to_nhwc: null pointer"); return ADAIN_EINVAL; }
    return launch_nchw_to_nhwc(in, out, n, c, hw, (hipStream_t)stream);
}

// ---- one sub-batch of the batch callers in one call ---------------------------------------------------------------------------
// Workspace of adain_stylize_u8: the blocks in the order they are taken, offsets in bytes.  A block the call does not use has no
// bytes and the offset ABSENT, which block() turns into a null pointer - how the blend knows that there is no depth map.
constexpr size_t ABSENT = ~(size_t)0;
static size_t take(Carve& c, size_t bytes) { return bytes ? c.take(bytes) : ABSENT; }
struct StylizePlan {
    int hc, wc, H8, W8;               // relu4_1 map; decoder output size (8hc x 8wc)
    int identity;                     // mask, decoder output and frame share one size: the fused composite + quantise tail
    int mask_only;                    // decoder output and frame share one size, the mask has another: the same tail sampling the mask
    size_t conv_bytes, stats_ws_bytes, pmap_ws_bytes;      // the workspaces handed on to the encoder / decoder, mean_std and strength_map
    size_t conv, f, g, c_mean, c_std, stats_ws, pmap, pmap_ws, img, content, mask_f, mask_r, sty_r, comp, total;
};
static StylizePlan stylize_plan(int n, int h, int w, int use_depth, int mask_n, int mask_c, int mask_h, int mask_w, int mask_is_float) {
    StylizePlan p{};
    adain_encoded_size(h, w, &p.hc, &p.wc);
    p.H8 = 8 * p.hc; p.W8 = 8 * p.wc;
    if (mask_n > 0) {
        p.identity = mask_h == h && mask_w == w && p.H8 == h && p.W8 == w;
        p.mask_only = !p.identity && p.H8 == h && p.W8 == w;
    }
    const bool general = mask_n > 0 && !p.identity && !p.mask_only;      // the composite on float images at the frame's size
    const size_t enc = adain_encode_workspace_bytes(n, h, w), dec = adain_decode_workspace_bytes(n, p.hc, p.wc);
    const size_t map = (size_t)n * p.hc * p.wc * sizeof(float), frame = (size_t)n * 3 * h * w * sizeof(float);
    p.conv_bytes = enc > dec ? enc : dec;
    p.stats_ws_bytes = mean_std_workspace_bytes(1, n, 512, p.hc * p.wc);
    p.pmap_ws_bytes = use_depth ? strength_map_workspace_bytes(p.hc, p.wc) : 0;
    Carve c;
    p.conv = take(c, p.conv_bytes);
    p.f = take(c, 512 * map);
    p.g = take(c, 512 * map);
    p.c_mean = take(c, (size_t)n * 512 * sizeof(float));
    p.c_std = take(c, (size_t)n * 512 * sizeof(float));
    p.stats_ws = take(c, p.stats_ws_bytes);
    p.pmap = take(c, use_depth ? map : 0);
    p.pmap_ws = take(c, p.pmap_ws_bytes);
    p.img = take(c, (size_t)n * 3 * p.H8 * p.W8 * sizeof(float));
    p.content = take(c, general ? frame : 0);
    p.mask_f = take(c, general && !mask_is_float ? (size_t)mask_n * mask_c * mask_h * mask_w * sizeof(float) : 0);
    p.mask_r = take(c, general && !(mask_h == h && mask_w == w) ? (size_t)mask_n * mask_c * h * w * sizeof(float) : 0);
    p.sty_r = take(c, general && !(p.H8 == h && p.W8 == w) ? frame : 0);
    p.comp = take(c, general ? frame : 0);
    p.total = c.at;
    return p;
}

size_t adain_stylize_u8_workspace_bytes(int n, int h, int w, int use_depth, int mask_n, int mask_c, int mask_h, int mask_w, int mask_is_float) {
    if (n < 1 || h < 9 || w < 9) return 0;
    return stylize_plan(n, h, w, use_depth, mask_n, mask_c, mask_h, mask_w, mask_is_float).total;
}

void adain_stylize_u8_out_size(int h, int w, int has_mask, int* oh, int* ow) {
    int hc, wc;
    adain_encoded_size(h, w, &hc, &wc);
    if (oh) *oh = has_mask ? h : 8 * hc;
    if (ow) *ow = has_mask ? w : 8 * wc;
}

size_t adain_stylize_u8_ex_workspace_bytes(int n, int h, int w, int use_depth, int mask_n, int mask_c, int mask_h, int mask_w, int mask_is_float) {
    return adain_stylize_u8_workspace_bytes(n, h, w, use_depth, mask_n, mask_c, mask_h, mask_w, mask_is_float);
}

static_assert(MIX_MAX_STYLES == ADAIN_MIX_MAX_STYLES, "csrc/common.h and include/adain_hip.h disagree");

// adain_stylize_u8 / _ex (one style, or one per frame) and adain_stylize_u8_mix (a weighted mix of k styles): style's rows are [512]
static int stylize_impl(const uint8_t* frames, int n, int h, int w, const float* enc_packed, const float* dec_packed, const StyleTerm& style,
                        float alpha, float one_minus_alpha, const float* const* depth_maps, const int* depth_h, const int* depth_w, float depth_offset,
                        float depth_prominence, const void* mask, int mask_is_float, int mask_n, int mask_c, int mask_h, int mask_w, uint8_t* out_u8,
                        void* workspace, size_t ws_bytes, adain_stream_t stream) {
    if (!frames || !enc_packed || !dec_packed || !style.s_mean || !style.s_std || !out_u8 || !workspace) { set_error("stylize_u8: null pointer"); return ADAIN_EINVAL; }
    if (n < 1 || h < 9 || w < 9) { set_error("stylize_u8: frames %dx%d too small (needs h, w >= 9)", h, w); return ADAIN_EINVAL; }
    if (!depth_maps && !(alpha >= 0.f && alpha <= 1.f)) { set_error("stylize_u8: alpha %g outside [0, 1]", alpha); return ADAIN_EINVAL; }   // test.py:75
    if (depth_maps && (!depth_h || !depth_w)) { set_error("stylize_u8: depth maps without their sizes"); return ADAIN_EINVAL; }
    if (depth_maps && !(depth_offset >= 0.f && depth_offset <= 1.f)) { set_error("stylize_u8: offset %g outside [0, 1]", depth_offset); return ADAIN_EINVAL; }   // test.py:56
    if (depth_maps)         // every argument is checked before the first launch: an error return leaves nothing queued on the stream
        for (int i = 0; i < n; ++i) {
            if (!depth_maps[i]) { set_error("stylize_u8: depth map %d is null", i); return ADAIN_EINVAL; }
            if (depth_h[i] < 1 || depth_w[i] < 1) { set_error("stylize_u8: depth map %d is %dx%d", i, depth_h[i], depth_w[i]); return ADAIN_EINVAL; }
        }
    if (!mask) mask_n = 0;
    if (mask && ((mask_n != 1 && mask_n != n) || (mask_c != 1 && mask_c != 3) || mask_h < 1 || mask_w < 1)) {
        set_error("stylize_u8: mask [%d][%d][%d][%d] does not fit %d RGB frames", mask_n, mask_c, mask_h, mask_w, n);
        return ADAIN_EINVAL;
    }
    // launch_mask_to_f32's limit (a thread per element), here with the other arguments: it runs behind the encoder, the blend and the decoder
    if (mask && !mask_is_float && (size_t)mask_n * mask_c * mask_h * mask_w > 0xffffff00ULL) {
        set_error("stylize_u8: a uint8 mask of more than 2^32 - 256 elements");
        return ADAIN_EINVAL;
    }
    const StylizePlan p = stylize_plan(n, h, w, depth_maps != nullptr, mask_n, mask_c, mask_h, mask_w, mask_is_float);
    RET_IF(check_workspace("stylize_u8", workspace, ws_bytes, p.total, 1));
    hipStream_t s = (hipStream_t)stream;
    auto block = [workspace](size_t offset) { return offset == ABSENT ? nullptr : (float*)((char*)workspace + offset); };
    float *conv = block(p.conv), *f = block(p.f), *g = block(p.g), *c_mean = block(p.c_mean), *c_std = block(p.c_std), *stats_ws = block(p.stats_ws);
    float *pmap = block(p.pmap), *pmap_ws = block(p.pmap_ws), *img = block(p.img);
    float *content_f = block(p.content), *mask_f = block(p.mask_f), *mask_r = block(p.mask_r), *sty_r = block(p.sty_r), *comp = block(p.comp);
    const int hw_c = p.hc * p.wc;
    const BlendTerm blend{alpha, one_minus_alpha, pmap, n};      // pmap: null without depth maps
    if (check_adain_blend("stylize_u8", 1, n, 512, hw_c, style, blend)) return ADAIN_EINVAL;     // the blend's own rules, on the relu4_1 map's size

    // vgg(content) with ToTensor inside the first layer (test.py:203-204, :57 / :76), calc_mean_std(content_f) (function.py:4-12)
    RET_IF(adain_encode_u8(frames, f, enc_packed, conv, p.conv_bytes, n, h, w, nullptr, stream));
    RET_IF(launch_mean_std(f, 1, n, 512, hw_c, 1e-5f, c_mean, c_std, stats_ws, p.stats_ws_bytes, s));
    if (depth_maps)         // compute_stylization_strength_map per frame (test.py:66-69)
        for (int i = 0; i < n; ++i) {
            RET_IF(launch_strength_map(depth_maps[i], depth_h[i], depth_w[i], p.hc, p.wc, depth_offset, depth_prominence, pmap + (size_t)i * hw_c,
                                       pmap_ws, p.pmap_ws_bytes, s));
        }
    // AdaIN * (1 - P) + content_f * P (test.py:70) or AdaIN * alpha + content_f * (1 - alpha) (test.py:79-80), AdaIN of the one style,
    // the frame's own, or the weighted mix of k (test_video.py:36-44)
    RET_IF(launch_adain_blend(f, 1, n, 512, hw_c, c_mean, c_std, style, blend, g, s));
    if (mask_n == 0 && ((uintptr_t)out_u8 & 3) == 0)        // decoder with save_image's quantiser inside its last layer (test.py:71 / :81, :243-244): the finished uint8 frames
        return decode_impl(g, nullptr, out_u8, dec_packed, conv, p.conv_bytes, n, p.hc, p.wc, nullptr, stream);
    RET_IF(adain_decode(g, img, dec_packed, conv, p.conv_bytes, n, p.hc, p.wc, nullptr, stream));     // test.py:71 / :81
    if (mask_n == 0) return launch_quantize_u8(img, out_u8, n, 3, p.H8, p.W8, s);                                // test.py:243-244 (unaligned output)
    if (p.identity)         // both F.interpolate calls of test.py:227-234 are identities: composite + quantise in one pass
        return launch_composite_quantize_u8(frames, img, mask, mask_is_float, mask_c, mask_n, out_u8, n, h * w, s);
    if (p.mask_only)        // only the mask needs its nearest resize: an index map, sampled in place by the same fused tail
        return launch_composite_quantize_u8_nearest(frames, img, mask, mask_is_float, mask_c, mask_n, mask_h, mask_w, out_u8, n, h, w, s);
    // the general composite (test.py:222-236): mask.float() -> nearest to the frame size; output -> bilinear to the frame size
    RET_IF(launch_u8_to_f32(frames, content_f, n, 3, h, w, s));
    const float* m = (const float*)mask;
    if (!mask_is_float) {
        RET_IF(launch_mask_to_f32((const uint8_t*)mask, mask_f, (size_t)mask_n * mask_c * mask_h * mask_w, s));
        m = mask_f;
    }
    if (mask_r) {
        RET_IF(launch_resize_nearest(m, mask_r, mask_n * mask_c, mask_h, mask_w, h, w, s));
        m = mask_r;
    }
    const float* sty = img;
    if (sty_r) {
        RET_IF(launch_resize_bilinear(img, sty_r, n * 3, p.H8, p.W8, h, w, s));
        sty = sty_r;
    }
    RET_IF(launch_mask_composite(content_f, sty, m, mask_c, mask_n, comp, n, 3, h * w, s));
    return launch_quantize_u8(comp, out_u8, n, 3, h, w, s);
}

int adain_stylize_u8(const uint8_t* frames, int n, int h, int w, const float* enc_packed, const float* dec_packed, const float* s_mean,
                     const float* s_std, float alpha, float one_minus_alpha, const float* const* depth_maps, const int* depth_h, const int* depth_w,
                     float depth_offset, float depth_prominence, const void* mask, int mask_is_float, int mask_n, int mask_c, int mask_h,
                     int mask_w, uint8_t* out_u8, void* workspace, size_t ws_bytes, adain_stream_t stream) {
    return stylize_impl(frames, n, h, w, enc_packed, dec_packed, StyleTerm{s_mean, s_std, 1, 0, nullptr, 1, 1}, alpha, one_minus_alpha, depth_maps, depth_h,
                        depth_w, depth_offset, depth_prominence, mask, mask_is_float, mask_n, mask_c, mask_h, mask_w, out_u8, workspace, ws_bytes, stream);
}

// s_mean / s_std [style_n][512], style_n 1 (adain_stylize_u8) or n: one style per frame
int adain_stylize_u8_ex(const uint8_t* frames, int n, int h, int w, const float* enc_packed, const float* dec_packed, const float* s_mean,
                        const float* s_std, int style_n, float alpha, float one_minus_alpha, const float* const* depth_maps, const int* depth_h,
                        const int* depth_w, float depth_offset, float depth_prominence, const void* mask, int mask_is_float, int mask_n, int mask_c,
                        int mask_h, int mask_w, uint8_t* out_u8, void* workspace, size_t ws_bytes, adain_stream_t stream) {
    if (style_n != 1 && style_n != n) { set_error("stylize_u8: %d styles for %d frames (1 or one per frame)", style_n, n); return ADAIN_EINVAL; }
    return stylize_impl(frames, n, h, w, enc_packed, dec_packed, StyleTerm{s_mean, s_std, 1, style_n == n, nullptr, 1, 1}, alpha, one_minus_alpha, depth_maps,
                        depth_h, depth_w, depth_offset, depth_prominence, mask, mask_is_float, mask_n, mask_c, mask_h, mask_w, out_u8, workspace, ws_bytes,
                        stream);
}

size_t adain_stylize_u8_mix_workspace_bytes(int n, int h, int w, int use_depth, int mask_n, int mask_c, int mask_h, int mask_w, int mask_is_float) {
    return adain_stylize_u8_workspace_bytes(n, h, w, use_depth, mask_n, mask_c, mask_h, mask_w, mask_is_float);
}

// s_mean / s_std [k][512] mixed by weights [weights_n][k][weights_hw] (adain_blend_mix in place of adain_blend_alpha / _pmap)
int adain_stylize_u8_mix(const uint8_t* frames, int n, int h, int w, const float* enc_packed, const float* dec_packed, const float* s_mean,
                         const float* s_std, int k, const float* weights, int weights_n, int weights_hw, float alpha, float one_minus_alpha,
                         const float* const* depth_maps, const int* depth_h, const int* depth_w, float depth_offset, float depth_prominence,
                         const void* mask, int mask_is_float, int mask_n, int mask_c, int mask_h, int mask_w, uint8_t* out_u8, void* workspace,
                         size_t ws_bytes, adain_stream_t stream) {
    if (!weights) { set_error("stylize_u8_mix: null pointer"); return ADAIN_EINVAL; }
    return stylize_impl(frames, n, h, w, enc_packed, dec_packed, StyleTerm{s_mean, s_std, k, 0, weights, weights_n, weights_hw}, alpha, one_minus_alpha,
                        depth_maps, depth_h, depth_w, depth_offset, depth_prominence, mask, mask_is_float, mask_n, mask_c, mask_h, mask_w, out_u8, workspace,
                        ws_bytes, stream);
}

size_t adain_coral_workspace_bytes(int n, int style_n, int hs, int ws, int hc, int wc) { return coral_workspace_bytes(n, style_n, hs, ws, hc, wc); }

int adain_coral(const void* style, int style_is_u8, int style_n, int hs, int ws, const void* content, int content_is_u8, int n, int hc, int wc,
                float* out, void* workspace, size_t ws_bytes, adain_stream_t stream) {
    return launch_coral(style, style_is_u8, style_n, hs, ws, content, content_is_u8, n, hc, wc, out, workspace, ws_bytes, (hipStream_t)stream);
}

size_t adain_conv3x3_wino4_packed_floats(int cin, int cout) { return (size_t)cin * cout * 24; }

int adain_conv3x3_wino4_pack(const float* w, float* packed, int cin, int cout, adain_stream_t stream) {
    if (!w || !packed) { set_error("conv3x3_wino4_pack: null pointer"); return ADAIN_EINVAL; }
    return launch_pack_wino4(w, packed, cin, cout, (hipStream_t)stream);
}

int adain_conv3x3_wino(const float* in, float* out, const float* packed_w, const float* bias, int n, int h, int w, int hs, int ws,
                       int cin, int cout, int src_mode, int relu, int pool_out, int mh, adain_stream_t stream) {
    if (!in || !out || !packed_w || !bias) { set_error("conv3x3_wino: null pointer"); return ADAIN_EINVAL; }
    ConvArgs a{};
    a.in = in; a.out = out; a.wpk = packed_w; a.bias = bias;
    a.n = n; a.H = h; a.W = w; a.Hs = hs; a.Ws = ws; a.cin = cin; a.cout = cout; a.relu = relu; a.pool_out = pool_out ? 1 : 0;
    if (mh != 5) {      // F(4,3) x F(2,3), weights packed by adain_conv3x3_wino4_pack: the one form this library holds
        set_error("conv3x3_wino: form %d is retired (rounds 1-2: F(2x2,3x3) forms 1-4); this library runs form 5, F(4,3) x F(2,3)", mh);
        return ADAIN_EINVAL;
    }
    return launch_conv3x3_wino4(a, src_mode, (hipStream_t)stream);
}

size_t adain_conv3x3_wino4_split_workspace_bytes(int n, int h, int w, int cin, int cout) {
    return wino4_split_floats(n, h, w, cin, cout) * sizeof(float);
}

size_t adain_conv3x3_up2x_poly_packed_floats(int cin, int cout) { return (size_t)cin * cout * 96; }

int adain_conv3x3_up2x_poly_pack(const float* w, float* packed, int cin, int cout, adain_stream_t stream) {
    if (!w || !packed) { set_error("conv3x3_up2x_poly_pack: null pointer"); return ADAIN_EINVAL; }
    return launch_pack_up2x_poly(w, packed, cin, cout, (hipStream_t)stream);
}

int adain_conv3x3_up2x_poly(const float* in, float* out, const float* packed_w, const float* bias, int n, int hs, int ws, int cin, int cout,
                            int relu, adain_stream_t stream) {
    if (!in || !out || !packed_w || !bias) { set_error("conv3x3_up2x_poly: null pointer"); return ADAIN_EINVAL; }
    ConvArgs a{};
    a.in = in; a.out = out; a.wpk = packed_w; a.bias = bias;
    a.n = n; a.Hs = hs; a.Ws = ws; a.H = 2 * hs; a.W = 2 * ws; a.cin = cin; a.cout = cout; a.relu = relu;
    return launch_conv3x3_up2x_poly(a, (hipStream_t)stream);
}

int adain_conv3x3_wino4_split(const float* in, float* out, const float* packed_w, const float* bias, int n, int h, int w, int hs, int ws,
                              int cin, int cout, int src_mode, int relu, int pool_out, void* workspace, size_t ws_bytes, adain_stream_t stream) {
    if (!in || !out || !packed_w || !bias) { set_error("conv3x3_wino4_split: null pointer"); return ADAIN_EINVAL; }
    ConvArgs a{};
    a.in = in; a.out = out; a.wpk = packed_w; a.bias = bias;
    a.n = n; a.H = h; a.W = w; a.Hs = hs; a.Ws = ws; a.cin = cin; a.cout = cout; a.relu = relu; a.pool_out = pool_out ? 1 : 0;
    return launch_conv3x3_wino4(a, src_mode, (hipStream_t)stream, SplitWs{(float*)workspace, workspace ? ws_bytes / sizeof(float) : 0});
}

}  // extern "C"
