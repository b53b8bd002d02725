/*
 * fsr_hip.h -- C ABI of libfsr_hip.so, the MI355X (gfx950) kernel library behind the
 * Fast-SRGAN drop-in modules (Generator / Discriminator / VGG19 / Trainer / NumpyImagesDataset).
 *
 * The reference (HasnainRaz/Fast-SRGAN) has no FFI layer: every hot-path operator is a stock
 * torch.nn call.  Each entry point below therefore cites the reference call site(s) whose
 * arithmetic it replaces (paths relative to /root/reference).  The binding a maintainer would
 * add on the reference side is a ctypes stub; see INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer borrowed from the caller (a torch tensor's data_ptr());
 *     the library never allocates, frees or synchronises; calls only enqueue work on `stream`
 *     (a hipStream_t passed as void*), so they are legal inside hipGraph stream capture;
 *   - activations are NHWC; `dtype` is the storage type of activations, activation gradients and
 *     packed filters: FSR_F32 (exact-f32 MFMA, parity mode), FSR_BF16 (bf16 MFMA, f32 accumulate) or
 *     FSR_F16 (fp16 MFMA, f32 accumulate: BASELINE configs[4]); parameters, biases, statistics,
 *     parameter gradients and losses are float;
 *   - FSR_X3 ("split bf16", the fast mode INSIDE the reference's fp32 tolerance): an element is 4 bytes, the pair
 *     hi = bf16(v), lo = bf16(v - hi), and every product of a convolution is three bf16 MFMAs into one f32 accumulator,
 *     x_hi*w_hi + x_lo*w_hi + x_hi*w_lo (the dropped x_lo*w_lo term is <= 2^-16 of the product).  Storage: an NHWC tensor of
 *     C channels (C %% 32 == 0) holds, per pixel and per group of 32 channels, 64 bytes of hi[32] followed by 64 bytes of
 *     lo[32] -- the same bytes as float32 (the torch container IS a float32 tensor of the logical shape), and to the MFMA
 *     kernels a bf16 tensor of 2C channels whose 32-channel chunks alternate hi / lo.  Tensor bases are 128-byte aligned.
 *     Packed filters are bf16 [9][rows][2K] with the same hi / lo chunk order along K.  Everything that is float in the
 *     other modes (parameters, statistics, gradients of parameters, losses, 3-channel images) is float here too;
 *   - channel counts of NHWC activations are multiples of FSR_CPAD(dtype) = 16 (f32) / 32 (bf16, f16, x3);
 *     3-channel images are stored zero-padded to that width;
 *   - reductions over pixels (InstanceNorm statistics, backward sums, bias / PReLU-slope gradients, loss
 *     means) are two-level and ORDER-FIXED: the producing kernel stores one partial vector per workgroup into
 *     the caller's `scratch` buffer (size from the matching fsr_*_scratch query; contents are don't-care before
 *     and after the call, the buffer may be reused by the next call on the same stream), and a second
 *     kernel enqueued by the same call adds the partials in a fixed order and ASSIGNS the result.  There are
 *     no float atomics anywhere: the same inputs give the same bits on every run.  Only the weight gradients
 *     (`dw_oihw`, and the `dbias` of fsr_conv3x3_c3_wgrad) ACCUMULATE into their outputs ("+=", one thread
 *     per element): the caller zeroes them once per optimizer step;
 *   - return value 0 = enqueued, < 0 = rejected (nothing enqueued); fsr_last_error() gives the
 *     reason for the calling thread.  The functions are thread-compatible.
 */
#ifndef FSR_HIP_H
#define FSR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSR_ABI_VERSION 16

enum { FSR_F32 = 0, FSR_BF16 = 1, FSR_F16 = 2, FSR_X3 = 3 };
enum { FSR_ACT_NONE = 0, FSR_ACT_RELU = 1, FSR_ACT_LEAKY = 2, FSR_ACT_PRELU = 3, FSR_ACT_TANH = 4 };
enum { FSR_CONV_FWD = 0, FSR_CONV_DGRAD = 1 };
enum { FSR_PACK_FWD = 0, FSR_PACK_FWD_PS = 1, FSR_PACK_DGRAD = 2, FSR_PACK_DGRAD_PS = 3 };
enum { FSR_OUT_DTYPE = 0, FSR_OUT_F32 = 1, FSR_OUT_U8 = 2, FSR_OUT_I420 = 3, FSR_OUT_NV12 = 4 };   /* fsr_conv_desc.out_f32 */
enum { FSR_YUV_BT601 = 0, FSR_YUV_BT709 = 1 };             /* fsr_conv_desc.yuv_matrix, fsr_i420_to_image */
enum { FSR_SITING_JPEG = 0, FSR_SITING_MPEG2 = 1 };        /* chroma siting of fsr_i420_to_image's input */
enum { FSR_CHROMA_420 = 0, FSR_CHROMA_422 = 1, FSR_CHROMA_444 = 2 };   /* chroma subsampling of the fsr_*_yuv entry points */
enum { FSR_LAYOUT_PLANAR = 0, FSR_LAYOUT_NV12 = 1 };       /* payload layout of the fsr_*_yuv_ex entry points */

typedef void* fsr_stream_t; /* hipStream_t */

int fsr_version(void);
const char* fsr_last_error(void);
/* Name of the kernel configuration the calling thread's most recent fsr_conv3x3 dispatched (profiling aid). */
const char* fsr_last_kernel(void);
/* "name=<marketing name>;arch=<gcnArchName>;cus=<n>;hbm_bytes=<n>" of the current device. */
int fsr_device_info(char* buf, size_t buflen);

/* ------------------------------------------------------------------ filter packing
 * torch Conv2d weights are OIHW float (state_dict layout, model.py:30-35,47-64,...).  The
 * kernels consume [9 taps][rows_pad][K_pad] in `dtype` with K contiguous:
 *   FSR_PACK_FWD       rows = cout, K = cin                  slice index = ky*3+kx
 *   FSR_PACK_FWD_PS    as FWD, rows permuted r = (co%4)*(cout/4) + co/4 so that the epilogue of
 *                      the PixelShuffle(2) convs (model.py:36,40) stores contiguous channels
 *   FSR_PACK_DGRAD     rows = cin,  K = cout                 (transposed filter for dL/dx)
 *   FSR_PACK_DGRAD_PS  as DGRAD with K permuted like FWD_PS rows
 * rows_pad = rows rounded up to 16 (head conv, model.py:103-108; first-layer data gradients:
 * 3 -> 16); K_pad = `k_pad` >= K (3-channel inputs: K zero-padded to FSR_CPAD).  Padding is zero
 * filled.  `packed` holds 9*rows_pad*k_pad elements. */
int fsr_pack_conv3x3(int dtype, int mode, const float* w_oihw, int cout, int cin, int k_pad, void* packed,
                     fsr_stream_t stream);
/* The same four layouts, STAGE-CONTIGUOUS for the 128..512-channel kernels (16-bit dtypes; rows a multiple of `block` = 64 or
 * 128, K a multiple of 32, no padding): [rows / block][K / 32][9 slices][block rows][32 channels], the rows of a block in the
 * kernels' LDS order and the 16-byte units of a 32-channel chunk XOR-swizzled as they lie in LDS, so the LDS-DMA of one
 * (block, chunk, slice) reads block * 64 contiguous bytes (whole 128-byte lines) instead of half lines 2 K bytes apart.
 * Which launches take it: fsr_conv3x3_pack_block().  `packed` holds 9 * rows * K elements. */
int fsr_pack_conv3x3_lin(int dtype, int mode, const float* w_oihw, int cout, int cin, int block, void* packed,
                         fsr_stream_t stream);

/* ------------------------------------------------------------------ 3x3 convolution, pad 1
 * Forward:  torch.nn.Conv2d(k=3, p=1, stride 1|2) at model.py:47-64, 86-93, 30-35, 103-108,
 *           124-131, 148-183 and vgg19.features convs (model.py:8), fused with the bias add, an
 *           activation (ReLU model.py:8 / LeakyReLU model.py:133,145 / PReLU model.py:37 /
 *           Tanh model.py:109), PixelShuffle(2) (model.py:36) and the per-(n,c) sum / sum of
 *           squares InstanceNorm2d (model.py:55,65,94,132) needs.
 * Dgrad:    the same kernel on the transposed filter: dL/dx of those convolutions.
 *   mode FSR_CONV_FWD  : in [n,ih,iw,cin] -> out [n,oh,ow,cout], oh = (ih-1)/stride+1
 *   mode FSR_CONV_DGRAD: in = dL/dy [n,ih,iw,cin], out = dL/dx [n,oh,ow,cout] where
 *                        (ih,iw,cin) are the forward OUTPUT dims and (oh,ow,cout) the forward
 *                        INPUT dims; stride is the forward stride.
 * cin is the (padded) channel count of `in` and the K_pad of the packed filter.
 * pixel_shuffle (FWD): out is [n,2oh,2ow,cout/4]; filters packed FSR_PACK_FWD_PS.
 * in_pixel_shuffled (DGRAD): in is [n,2ih,2iw,cin/4]; filters packed FSR_PACK_DGRAD_PS.
 * out_f32: FSR_OUT_DTYPE (0): `dtype` output; FSR_OUT_F32 (1): store float whatever `dtype` is (3-channel outputs:
 *   head images, image gradients); FSR_OUT_U8 (2, FSR_ACT_TANH heads, forward): store the uint8 HWC image
 *   (unsigned char)(((tanh(z) + 1) / 2) * 255) -- inference.py:53-56's post-processing with its truncating cast,
 *   out [n,oh,ow,cout] bytes (cout = 3: the finished RGB frame); FSR_OUT_I420 (3, FSR_ACT_TANH heads, forward, stride 1,
 *   cout = 3, even oh and ow, no statistics / pre-activation / mask / scale tensors): store the I420 (planar YUV 4:2:0) frame of the
 *   RGB head output -- per image the Y plane [oh][ow], then Cb and Cr [oh/2][ow/2] (oh * ow * 3 / 2 bytes, C420jpeg siting:
 *   chroma is the mean of the 2x2 block), matrix and range from yuv_matrix / yuv_full_range; FSR_OUT_NV12 (4, ABI 16; the
 *   conditions of FSR_OUT_I420): the same codes as the NV12 frame -- the Y plane, then ONE plane [oh/2][ow/2] of (Cb, Cr) byte pairs.
 * pool2 (inference / no-grad passes of vgg19.features, model.py:8,191): the kernel's epilogue takes the 2x2 maximum of the
 *   activated outputs and stores only the pooled tensor -- the full-resolution tensor, which only a backward pass would
 *   read, is never written.  oh, ow even; cout %% 16 == 0; no stats / preact / mask tensors.
 * stats (optional): float [n][cout][2]; receives the sum and the sum of squares of the pre-activation
 *   over pixels (needs `scratch` of fsr_conv3x3_scratch(desc) bytes; FWD and stride-1 DGRAD launches).
 * preact (optional): tensor like out; receives the pre-activation (training: PReLU backward
 *   needs its sign, which the output of a negative-slope PReLU does not reveal).
 * oscale (optional): float [cout] multiplied into the result before bias/activation (the
 *   1/(2 std) of VGG19.forward's normalisation, model.py:21-22, applied to input gradients).
 * dact_mask (optional): tensor like out; the result is multiplied by (mask > 0 ? 1 : dact_slope).  A
 *   data-gradient launch uses it to apply the ReLU / LeakyReLU backward of the layer that PRODUCED the
 *   forward input (mask = that layer's output), saving a separate elementwise pass.
 *   With desc.mask_is_addend the same tensor is ADDED to the result instead (before the activation): the data gradient of
 *   the first convolution of a ResidualBlock (model.py:67-69) takes the gradient of the block's skip connection there, so
 *   dL/dx = conv_dgrad(dz) + dL/d(skip) leaves the kernel in one piece and autograd has nothing to accumulate (round 2 ran
 *   nine at::add<bf16> kernels per iteration for this). */
typedef struct fsr_conv_desc {
  int dtype;
  int mode;
  int n, ih, iw, cin;
  int oh, ow, cout;
  int stride;
  int act;
  float slope;
  int pixel_shuffle;
  int in_pixel_shuffled;
  int out_f32;
  int pool2; /* FWD, 16-bit dtypes, no pixel shuffle: out is the MaxPool2d(2,2) of the activated result, [n,oh/2,ow/2,cout] */
  int mask_is_addend; /* 0: dact_mask gates the result by its sign; 1: it is ADDED to the result instead (see below); 2 (stride-2 data
                         gradients, 16-bit dtypes and FSR_X3): it is the PACKED SIGN-BIT tensor [n][oh][ow][cout / 8] of the producing layer's output
                         (bit c & 7 of byte c >> 3 = output > 0: fsr_conv3x3_c3_fwd's `signs`), gating like 0 at a sixteenth of the bytes */
  int pack_lin; /* 0: packed_w is fsr_pack_conv3x3's layout; 64 / 128: fsr_pack_conv3x3_lin's with that block (must equal fsr_conv3x3_pack_block) */
  int yuv_matrix;     /* FSR_OUT_I420 / FSR_OUT_NV12: FSR_YUV_BT601 or FSR_YUV_BT709 (ignored by the other output kinds) */
  int yuv_full_range; /* FSR_OUT_I420 / FSR_OUT_NV12: 0 limited range (Y 16..235, C 16..240), 1 full range (0..255) */
} fsr_conv_desc;

/* Block size of the stage-contiguous filter pack (fsr_pack_conv3x3_lin) that the kernel fsr_conv3x3 would dispatch for `desc`
 * reads, or 0 if it reads the standard pack (always a valid choice: every kernel also accepts pack_lin = 0).  The optional
 * tensors of the call take part in the dispatch: say which ones will be given.  Nothing is launched.  < 0: error. */
enum { FSR_OPT_BIAS = 1, FSR_OPT_PRELU = 2, FSR_OPT_OSCALE = 4, FSR_OPT_MASK = 8, FSR_OPT_PREACT = 16, FSR_OPT_STATS = 32 };
int fsr_conv3x3_pack_block(const fsr_conv_desc* desc, int optional_tensors);

size_t fsr_conv3x3_scratch(const fsr_conv_desc* desc);
int fsr_conv3x3(const fsr_conv_desc* desc, const void* in, const void* packed_w, const float* bias,
                const float* prelu_weight, const float* oscale, const void* dact_mask, float dact_slope, void* out,
                void* preact, float* stats, void* scratch, fsr_stream_t stream);

/* Weight gradient of the same convolutions: dW[co][ci][ky][kx] (OIHW float, torch .grad layout)
 *   += sum_{n,y,x} dy[n,y,x,co] * x[n, y*stride+ky-1, x*stride+kx-1, ci]      (autograd of model.py convs)
 * x [n,ih,iw,cin_pad], dy [n,oh,ow,cout_pad] (or [n,2oh,2ow,cout/4] when dy_pixel_shuffled).
 * Only dW[:cout][:cin] is written (cin/cout may be smaller than the padded tensor widths).
 * `workspace` (float, fsr_conv3x3_wgrad_workspace() bytes) holds split-K partials; dw accumulates. */
typedef struct fsr_wgrad_desc {
  int dtype;
  int n, ih, iw, cin_pad, cin;
  int oh, ow, cout_pad, cout;
  int stride;
  int dy_pixel_shuffled;
} fsr_wgrad_desc;
size_t fsr_conv3x3_wgrad_workspace(const fsr_wgrad_desc* desc);
int fsr_conv3x3_wgrad(const fsr_wgrad_desc* desc, const void* x, const void* dy, float* dw_oihw, void* workspace,
                      fsr_stream_t stream);
/* The same weight gradient for `nlayers` (1..32) layers of ONE shape in one launch: layer l reads x[l], dy[l] and
 * accumulates into dw_oihw[l] (host arrays of device pointers, read during the call only).  For the generator's 64 -> 64
 * 3x3 blocks (model.py:62-80; 17 identical layers at trainer.py:121-129's backward): cout = cin = 64 unpadded.
 * The layers share the launch's workgroups, so the split-K partials (workspace:
 * fsr_conv3x3_wgrad_grouped_workspace(desc, nlayers) bytes) shrink by the group size and one reduce serves all layers.
 * Summation order is fixed by (shape, nlayers): bit-reproducible, but not bit-equal to nlayers separate calls. */
size_t fsr_conv3x3_wgrad_grouped_workspace(const fsr_wgrad_desc* desc, int nlayers);
int fsr_conv3x3_wgrad_grouped(const fsr_wgrad_desc* desc, int nlayers, const void* const* x, const void* const* dy,
                              float* const* dw_oihw, void* workspace, fsr_stream_t stream);

/* ------------------------------------------------------------------ InstanceNorm2d (+ activation, + residual)
 * torch.nn.InstanceNorm2d defaults (model.py:55,65,94,132: biased variance, eps 1e-5, no affine)
 * applied to the raw conv output using the statistics the conv epilogue accumulated, fused with
 * PReLU (model.py:56) / LeakyReLU (model.py:133) and the residual add (model.py:69,115):
 *   out = act((x - mean) * rstd) + res.          x, res, out: [n,hw,c] `dtype`; stats [n][c][2]. */
int fsr_instnorm_act_fwd(int dtype, const void* x, const float* stats, const void* res, int act, float slope,
                         const float* prelu_weight, void* out, int n, int hw, int c, fsr_stream_t stream);
/* Backward, phase 1: sums[n][c][2] = (sum gz, sum gz*xhat) with gz = g * act'(xhat);
 * dprelu[0] = sum g*min(xhat,0) (optional); scratch: fsr_instnorm_act_bwd_scratch(n,hw,c) bytes.
 * Phase 2: dx = rstd*(gz - mean(gz) - xhat*mean(gz*xhat)). */
size_t fsr_instnorm_act_bwd_scratch(int n, int hw, int c);
int fsr_instnorm_act_bwd_reduce(int dtype, const void* g, const void* x, const float* stats, int act, float slope,
                                const float* prelu_weight, float* sums, float* dprelu, void* scratch, int n, int hw,
                                int c, fsr_stream_t stream);
int fsr_instnorm_act_bwd_apply(int dtype, const void* g, const void* x, const float* stats, const float* sums,
                               int act, float slope, const float* prelu_weight, void* dx, int n, int hw, int c,
                               fsr_stream_t stream);

/* ------------------------------------------------------------------ activation backward of a fused conv epilogue
 * dz = g * act'(.) for the activations fsr_conv3x3 fuses; `saved` is the conv OUTPUT for
 * ReLU / LeakyReLU(slope > 0) and the saved PRE-activation for PReLU.  Tensors [n,h,w,c] `dtype`.
 * dbias (optional, float [cb]) = per-channel sums of dz; with pixel_shuffled != 0 the tensors are
 * the depth-to-space outputs of a cb = 4c channel conv and dbias index = 4*ch + 2*(y&1) + (x&1).
 * dprelu (optional) = sum g*min(saved,0).  dz may be null when only the reductions are wanted (bias gradient of a
 * layer whose activation backward was already applied by its consumer's data-gradient epilogue).
 * scratch (needed with dbias / dprelu): fsr_act_bwd_scratch(n,h,w,c,pixel_shuffled) bytes. */
size_t fsr_act_bwd_scratch(int n, int h, int w, int c, int pixel_shuffled);
int fsr_act_bwd(int dtype, const void* g, const void* saved, int act, float slope, const float* prelu_weight,
                void* dz, float* dbias, float* dprelu, void* scratch, int n, int h, int w, int c, int pixel_shuffled,
                fsr_stream_t stream);

/* out = a + b over `count` elements of `dtype` tensors of one layout (out may alias a): the gradient accumulation of an activation
 * with two consumers (the generator's long skip, model.py:115) -- in the x3 mode torch's own add cannot do it (the container's
 * float32 arithmetic is not the arithmetic of the pairs it holds). */
int fsr_add(int dtype, const void* a, const void* b, void* out, long long count, fsr_stream_t stream);

/* ------------------------------------------------------------------ 3-channel images <-> padded NHWC
 * img: float, element strides (sn, sc, sh, sw) -- any of NCHW (dataloader.py:36-38 tensors) or
 * NHWC (the head's output).  out[n,h,w,cpad] = img*scale[c] + shift[c] for c < 3, else 0.
 * (VGG19.forward's (x+1)/2, (x-mean)/std, model.py:21-22, is scale = 1/(2 std), shift = (0.5-mean)/std.) */
int fsr_image_to_nhwc(int dtype, const float* img, long long sn, long long sc, long long sh, long long sw, int n,
                      int h, int w, float scale0, float scale1, float scale2, float shift0, float shift1,
                      float shift2, void* out, int cpad, fsr_stream_t stream);
/* Head backward (model.py:102-110): dz = g * (1 - y^2) for y = tanh(z), written zero-padded NHWC;
 * g has element strides (sn,sc,sh,sw), y is the head output [n,h,w,3] float.  dbias[3] (optional) = sums;
 * scratch (with dbias): fsr_tanh_bwd_scratch() bytes.
 * fsr_tanh_bwd_image: the same gradient as a 3-channel float image dz [n,h,w,3] (no padding), for the first-layer kernels. */
size_t fsr_tanh_bwd_scratch(void);
int fsr_tanh_bwd_image(const float* g, long long sn, long long sc, long long sh, long long sw, const float* y_nhwc3, int n, int h,
                       int w, float* dz_nhwc3, float* dbias, void* scratch, fsr_stream_t stream);
int fsr_tanh_bwd_to_nhwc(int dtype, const float* g, long long sn, long long sc, long long sh, long long sw,
                         const float* y_nhwc3, int n, int h, int w, void* dz, int cpad, float* dbias, void* scratch,
                         fsr_stream_t stream);

/* uint8 HWC frames [n,h,w,3] -> float [n,h,w,3], x / 127.5 - 1 (inference.py:48: the first-layer kernels read the result
 * in place as an NCHW-shaped tensor of strides (3hw, 1, 3w, 3)). */
int fsr_u8_to_image(const uint8_t* frames, float* img, long long count, fsr_stream_t stream);

/* I420 frames (n contiguous payloads: Y [h][w], then Cb and Cr [(h+1)/2][(w+1)/2]; odd h and w are legal) -> float
 * [n,h,w,3] = 2 c - 1 of the decoded RGB c in [0, 1] -- the layout fsr_u8_to_image writes.  Chroma is upsampled bilinearly
 * (edge clamp) at the siting FSR_SITING_JPEG (centred on both axes) or FSR_SITING_MPEG2 (co-sited horizontally); `matrix`
 * FSR_YUV_BT601 / FSR_YUV_BT709, full_range 0 / 1. */
int fsr_i420_to_image(const uint8_t* frames, float* img, int n, int h, int w, int siting, int matrix, int full_range,
                      fsr_stream_t stream);

/* Deep samples (ABI 13): an I420 payload of depth 9 <= d <= 16 has the plane order and extents above with every
 * sample in 2 bytes, little-endian, the value in the low d bits (what Y4M C420p<d> carries) -- twice the bytes of an 8-bit payload.
 *   limited range: Y = (16 + 219 E_Y) 2^(d-8), C = (128 + 224 E_C) 2^(d-8);  full range: Y = (2^d - 1) E_Y, C = 2^(d-1) + (2^d - 1) E_C;
 *   encode: code = clamp(floor(v + 0.5), 0, 2^d - 1);  d = 8 gives the 8-bit numbers.
 * fsr_i420_to_image_deep: fsr_i420_to_image for such payloads (frames 2-byte aligned; depth outside 9..16 is refused; a stored value
 * above 2^d - 1 is taken as it is -- the clamp of R, G, B to [0, 1] deals with it). */
int fsr_i420_to_image_deep(const uint8_t* frames, float* img, int n, int h, int w, int siting, int matrix, int full_range, int depth,
                           fsr_stream_t stream);

/* The encode on its own: float tanh output t [n,h,w,3] (h, w even) -> n I420 payloads at `depth` 8..16 (uint8 samples for 8, 16-bit
 * samples above) -- c = clamp((t + 1) / 2, 0, 1), Y per pixel, Cb / Cr the mean of E_C over each 2x2 block (C420jpeg siting), the
 * arithmetic and summation order of fsr_conv3x3's FSR_OUT_I420 epilogue.  One streaming kernel; n * h * w stays below 2^31. */
int fsr_image_to_i420(const float* t, int n, int h, int w, int matrix, int full_range, int depth, void* out, fsr_stream_t stream);

/* 4:2:2 and 4:4:4 (ABI 14).  A planar payload is Y [h][w], then Cb, then Cr: [(h+1)/2][(w+1)/2] each for FSR_CHROMA_420 (the
 * I420 payload above), [h][(w+1)/2] for FSR_CHROMA_422, [h][w] for FSR_CHROMA_444; 1 byte per sample at depth 8, 2 (little-endian, the value
 * in the low d bits) at depth 9..16, where the payloads must be 2-byte aligned.  Matrices, ranges, codes and the clamp are those of 4:2:0.
 * fsr_yuv_to_image: n payloads (odd h and w are legal) -> float [n,h,w,3] = 2 c - 1.  4:4:4 has no interpolation and ignores `siting`;
 *   4:2:2 interpolates chroma horizontally only, linearly with edge clamp: luma column x reads chroma at x / 2 (FSR_SITING_MPEG2, what
 *   Y4M's C422 means) or (x - 1/2) / 2 (FSR_SITING_JPEG).  FSR_CHROMA_420 is fsr_i420_to_image / fsr_i420_to_image_deep.
 * fsr_image_to_yuv: float tanh output t [n,h,w,3] -> n payloads of c = clamp((t + 1) / 2, 0, 1).  Y per pixel; 4:4:4: Cb, Cr per pixel;
 *   4:2:2 (w even): chroma column j is co-sited with luma column 2j, E_C = ((d[2j-1] + d[2j+1]) + 2 d[2j]) / 4 / (2 (1 - K)) with d = B - E_Y
 *   or R - E_Y and columns -1 and w clamped to 0 and w - 1.  FSR_CHROMA_420 is fsr_image_to_i420 (h, w even).  n * h * w stays below 2^31.
 * Unknown chroma, depth outside 8..16, an odd 4:2:2 output width and misaligned 16-bit payloads are refused. */
int fsr_yuv_to_image(const uint8_t* frames, float* img, int n, int h, int w, int chroma, int siting, int matrix, int full_range, int depth,
                     fsr_stream_t stream);
int fsr_image_to_yuv(const float* t, int n, int h, int w, int chroma, int matrix, int full_range, int depth, void* out, fsr_stream_t stream);

/* Semi-planar 4:2:0 (ABI 16): `layout` FSR_LAYOUT_PLANAR is the call above; FSR_LAYOUT_NV12 (FSR_CHROMA_420 only) is the payload
 * hardware decoders produce -- Y [h][w], then ONE plane of [(h+1)/2] rows of [(w+1)/2] (Cb, Cr) pairs, Cb first; 1 byte per sample at depth 8
 * (NV12), 2 little-endian bytes at depth 9..16 with the code in the HIGH `depth` bits (P010, P012, P016): written with the low 16 - depth bits
 * zero, read as stored >> (16 - depth) whatever they hold.  The byte count is the planar payload's, and so is every code: matrices, ranges,
 * sitings, clamps, rounding and the order of the chroma sum are unchanged, only the addresses and the shift differ.  Refused: an unknown layout,
 * FSR_LAYOUT_NV12 with another chroma, and whatever the planar calls refuse (odd encode extents, depth outside 8..16, misaligned 16-bit
 * payloads).  NV21, NV16 / NV24 and pitched surfaces are not supported. */
int fsr_yuv_to_image_ex(const uint8_t* frames, float* img, int n, int h, int w, int chroma, int layout, int siting, int matrix, int full_range,
                        int depth, fsr_stream_t stream);
int fsr_image_to_yuv_ex(const float* t, int n, int h, int w, int chroma, int layout, int matrix, int full_range, int depth, void* out,
                        fsr_stream_t stream);

/* ------------------------------------------------------------------ arbitrary output size: antialiased bicubic resize of the head output
 * t: the head's float tanh output [n,h,w,3] (FSR_OUT_F32 of any dtype's head) -> an oh x ow image in ONE fused kernel (horizontal pass
 * of a tile's source-row window into LDS, vertical pass from LDS, conversion, store; no global intermediate, no atomics).  The
 * arithmetic is torch's upsample_bicubic2d_aa (F.interpolate(mode="bicubic", antialias=True, align_corners=False)) on c = (t + 1) / 2:
 *   v[yo][xo][ch] = sum_j wy[yo][j] * (sum_k wx[xo][k] * c[ymin[yo] + j][xmin[xo] + k][ch])      (float32, horizontal sum first)
 * wy float [oh][ky], ymin / ysize int [oh] and wx float [ow][kx], xmin / xsize int [ow] are the normalised tap tables of the two axes
 * (cubic a = -0.5; support 2 * max(in / out, 1); the tables of fsr_crop_resize, for any ratio in either direction).
 * out_kind: FSR_OUT_F32  float [n,oh,ow,3] = 2 v - 1, unclamped;
 *           FSR_OUT_U8   uint8 [n,oh,ow,3] = (unsigned char)(clamp(v, 0, 1) * 255) -- the truncating cast of fsr_conv3x3's FSR_OUT_U8, so
 *                        identity taps reproduce its bytes;
 *           FSR_OUT_I420 [n][oh * ow * 3 / 2] I420 payloads of clamp(v, 0, 1) (oh, ow even): Y per pixel, Cb / Cr the mean of E_C over each
 *                        2x2 block, C420jpeg siting, yuv_matrix / yuv_full_range as in fsr_conv_desc.
 * Any up-scaling factor; down-scaling up to h / oh <= 8 and w / ow <= 8 (ky, kx <= 33).  n * oh * ow and h * w stay below 2^31. */
int fsr_resample_image(const float* t, int n, int h, int w, int oh, int ow, const float* wy, const int* ymin, const int* ysize, int ky,
                       const float* wx, const int* xmin, const int* xsize, int kx, int out_kind, int yuv_matrix, int yuv_full_range,
                       void* out, fsr_stream_t stream);
/* ... with FSR_OUT_I420 planes of 16-bit samples at depth 9..16 (ABI 13; the deep payload of fsr_i420_to_image_deep): the same kernel
 * with a 16-bit code type in its I420 stage. */
int fsr_resample_image_i420_deep(const float* t, int n, int h, int w, int oh, int ow, const float* wy, const int* ymin, const int* ysize,
                                 int ky, const float* wx, const int* xmin, const int* xsize, int kx, int yuv_matrix, int yuv_full_range,
                                 int depth, void* out, fsr_stream_t stream);
/* ... with planar YUV payloads of `chroma` at depth 8..16 (ABI 14; the encode of fsr_image_to_yuv on clamp(v, 0, 1), identity taps reproduce
 * its bytes): any oh, ow for FSR_CHROMA_444, even ow for FSR_CHROMA_422; FSR_CHROMA_420 is the FSR_OUT_I420 stage above (oh, ow even). */
int fsr_resample_image_yuv(const float* t, int n, int h, int w, int oh, int ow, const float* wy, const int* ymin, const int* ysize, int ky,
                           const float* wx, const int* xmin, const int* xsize, int kx, int chroma, int yuv_matrix, int yuv_full_range,
                           int depth, void* out, fsr_stream_t stream);
/* ... with the payload `layout` of fsr_image_to_yuv_ex (ABI 16): FSR_LAYOUT_NV12 (FSR_CHROMA_420, oh and ow even) stores the semi-planar frame. */
int fsr_resample_image_yuv_ex(const float* t, int n, int h, int w, int oh, int ow, const float* wy, const int* ymin, const int* ysize, int ky,
                              const float* wx, const int* xmin, const int* xsize, int kx, int chroma, int layout, int yuv_matrix,
                              int yuv_full_range, int depth, void* out, fsr_stream_t stream);

/* ------------------------------------------------------------------ first-layer convolutions straight from the image
 * Conv2d(3 -> cout, k3, p1) of Generator.neck (model.py:75-78), Discriminator.neck (model.py:143-146) and
 * vgg19.features.0 (model.py:8, with VGG19.forward's normalisation model.py:20-22 folded in) without the padded
 * NHWC copy of the image: the kernels read img (float, element strides sn,sc,sh,sw) and use
 * round_dtype(img*scale[c] + shift[c]) -- the value fsr_image_to_nhwc would have stored -- as the conv input.
 * cout must be a multiple of 16.
 *   fsr_pack_conv3x3_c3 : OIHW float [cout][3][3][3] -> `dtype` [round_up(cout,16)][32], k = (ky*3+kx)*3 + ci.
 *   fsr_conv3x3_c3_fwd  : out[n,h,w,cout] = act(conv + bias); act NONE/RELU/LEAKY/PRELU; preact optional; signs optional (16-bit
 *                         dtypes and FSR_X3, cout % 64 == 0): uint8 [n,h,w,cout/8], bit c & 7 of byte c >> 3 = (out[..., c] > 0; FSR_X3:
 *                         the stored hi part > 0, the predicate the tensor mask applies) -- the activation-gradient mask of the layer as
 *                         fsr_conv3x3's mask_is_addend = 2 reads it.  The forward works in strips of 16, 32 or 64 rows (chosen per shape;
 *                         environment FSR_C3_ROWS = 16 | 32 | 64 forces one): results do not depend on the height.
 *   fsr_conv3x3_c3_wgrad: dw_oihw (float [cout][3][3][3]) += d loss / d weight for dz [n,h,w,cout] `dtype`;
 *                         dbias (optional, float [cout]) += per-channel sums of dz (the bias gradient: a column of
 *                         ones in the padded K dimension of the same MFMAs);
 *                         workspace of fsr_conv3x3_c3_wgrad_workspace(n,h,w,cout) bytes.
 * transposed != 0 serves the OTHER 3-channel end, the head Conv2d(cout -> 3) + Tanh (model.py:102-110), whose backward has the
 * same shape with the roles swapped -- img is then the 3-channel gradient dz = g (1 - y^2) (fsr_tanh_bwd_image):
 *   fsr_pack_conv3x3_c3(transposed): w_oihw is the head's [3][cout][3][3] filter; the pack holds its transposed, tap-flipped
 *                         form, and fsr_conv3x3_c3_fwd of `img` with it IS the head's data gradient [n,h,w,cout];
 *   fsr_conv3x3_c3_wgrad(transposed): `dz` is the head's 64-channel INPUT, dw_oihw the head's [3][cout][3][3] gradient. */
int fsr_pack_conv3x3_c3(int dtype, const float* w_oihw, int cout, void* packed, int transposed, fsr_stream_t stream);
int fsr_conv3x3_c3_fwd(int dtype, const float* img, long long sn, long long sc, long long sh, long long sw, int n, int h,
                       int w, float scale0, float scale1, float scale2, float shift0, float shift1, float shift2,
                       const void* packed_w, const float* bias, int act, float slope, const float* prelu_weight, int cout,
                       void* out, void* preact, void* signs, fsr_stream_t stream);
size_t fsr_conv3x3_c3_wgrad_workspace(int n, int h, int w, int cout);
int fsr_conv3x3_c3_wgrad(int dtype, const float* img, long long sn, long long sc, long long sh, long long sw, int n, int h,
                         int w, float scale0, float scale1, float scale2, float shift0, float shift1, float shift2,
                         const void* dz, int cout, float* dw_oihw, float* dbias, void* workspace, int transposed,
                         fsr_stream_t stream);

/* ------------------------------------------------------------------ MaxPool2d(2,2) of vgg19.features (model.py:8)
 * x [n,h,w,c] -> y [n,h/2,w/2,c].  Backward routes g to the first maximum in window scan order; with
 * relu_mask != 0 it also applies the backward of the ReLU that produced x (dx = 0 where x <= 0). */
/* argmax (optional, uint8 [n,h/2,w/2,c]): bits 0..1 = which of the four inputs of the window (row-major, the first one equal to the
 * maximum) was taken, bit 2 = maximum > 0; fsr_maxpool2_bwd_argmax needs nothing else of the forward pass. */
int fsr_maxpool2_fwd(int dtype, const void* x, void* y, void* argmax, int n, int h, int w, int c, fsr_stream_t stream);
int fsr_maxpool2_bwd_argmax(int dtype, const void* g, const void* argmax, void* dx, int n, int h, int w, int c, int relu_mask,
                            fsr_stream_t stream);
int fsr_maxpool2_bwd(int dtype, const void* g, const void* x, const void* y, void* dx, int n, int h, int w, int c,
                     int relu_mask, fsr_stream_t stream);

/* ------------------------------------------------------------------ Discriminator head: Conv2d(512 -> 1, k=1) (model.py:184-186)
 * logits[p] = b + sum_c x[p][c]*w[c]; x [npix,c] `dtype`, logits float.
 * Backward: dx[p][c] = g[p]*w[c]; dw[c] = sum_p g[p]*x[p][c]; db[0] = sum_p g[p];
 * scratch: fsr_conv1x1_c1_bwd_scratch(c) bytes. */
int fsr_conv1x1_c1_fwd(int dtype, const void* x, const float* w, const float* b, float* logits, int npix, int c,
                       fsr_stream_t stream);
size_t fsr_conv1x1_c1_bwd_scratch(int c);
int fsr_conv1x1_c1_bwd(int dtype, const float* g, const void* x, const float* w, void* dx, float* dw, float* db,
                       void* scratch, int npix, int c, fsr_stream_t stream);

/* ------------------------------------------------------------------ losses (trainer.py:41,43,177,178,188,192,109)
 * BCEWithLogitsLoss (mean): loss[0] = mean(max(x,0) - x*t + log1p(exp(-|x|))); x, t float [count];
 * scratch (both loss forwards): fsr_loss_scratch() bytes.
 * Backward: dx = gscale[0] * (sigmoid(x) - t) / count   (gscale: device scalar, the upstream grad). */
size_t fsr_loss_scratch(void);
int fsr_bce_logits_fwd(const float* x, const float* t, float* loss, void* scratch, long long count, fsr_stream_t stream);
int fsr_bce_logits_bwd(const float* x, const float* t, const float* gscale, float* dx, long long count,
                       fsr_stream_t stream);
/* SmoothL1Loss (beta 1, mean) between `a` and `b` (`dtype` tensors, or float when dtype_is_f32_io):
 * loss[0] = mean(huber(a-b)).  Backward: da = gscale[0]*clamp(a-b,-1,1)/count (db = -da not produced:
 * the target branch of trainer.py:191/:109 needs no gradient). */
int fsr_smooth_l1_fwd(int dtype, const void* a, const void* b, float* loss, void* scratch, long long count,
                      fsr_stream_t stream);
int fsr_smooth_l1_bwd(int dtype, const void* a, const void* b, const float* gscale, void* da, long long count,
                      fsr_stream_t stream);

/* ------------------------------------------------------------------ validation metrics (trainer.py:46-69)
 * torchmetrics' SSIM (gaussian 11x11, sigma 1.5, data_range 1.0, k1 .01, k2 .03; reflect padding + crop = only windows
 * entirely inside the image) and the squared error PSNR needs, for images a, b given in [-1,1] (the kernel applies
 * trainer.py:63-65's (1 + x) / 2): float tensors of logical shape [n,3,h,w] with element strides (sn,sc,sh,sw) each --
 * the generator's NHWC head output and the NCHW HR batch are both read in place.
 * out[n][2] = (sum over channels and valid pixels of the SSIM map, sum of squared errors over all pixels):
 *   SSIM_i = out[i][0] / (3 (h-10)(w-10));  PSNR = 10 log10(1 / (sum_i out[i][1] / (3 n h w))).
 * scratch: fsr_ssim_sse_scratch(n,h,w) bytes.  h, w > 10. */
size_t fsr_ssim_sse_scratch(int n, int h, int w);
int fsr_ssim_sse(const float* a, long long asn, long long asc, long long ash, long long asw, const float* b,
                 long long bsn, long long bsc, long long bsh, long long bsw, int n, int h, int w, float* out,
                 void* scratch, fsr_stream_t stream);

/* ------------------------------------------------------------------ benchmark quality on uint8 frames (added within ABI 16)
 * The evaluation protocol of the super-resolution literature, per image, in one launch: a, b are n images of h x w interleaved
 * RGB bytes (pixel stride 3), image i at a + i * a_image_bytes, row y at + y * a_row_bytes; the strides of a and b are
 * independent (one may be a contiguous batch, the other a cropped view of larger frames).  The region evaluated is rows
 * shave .. h - shave, columns shave .. w - shave (eh x ew); no byte outside it is read.  Values, float32 in code units 0..255:
 *   FSR_QUALITY_Y   : y = 16 + (65.481 r + 128.553 g + 24.966 b) / 255, the quotients (float)(65.481 / 255.0) etc. -- BT.601 studio luma
 *                     (evaluated as 16 + fma(kb, b, fma(kg, g, kr r)): the same bytes give the same value in a and in b);
 *   FSR_QUALITY_RGB : the three channels as they are.
 * out[i][1] = sum of squared differences over the region (one channel in Y mode, three in RGB mode);
 * out[i][0] = sum of the SSIM map (fsr_ssim_sse's window and formula, c1 = (0.01f * 255.f)^2, c2 = (0.03f * 255.f)^2) over the
 *             (eh - 10) x (ew - 10) windows inside the region and over the channels:
 *   PSNR_i = 10 log10(255^2 channels eh ew / out[i][1]);  SSIM_i = out[i][0] / (channels (eh - 10)(ew - 10)).
 * scratch: fsr_quality_u8_scratch(...) bytes (0 for n <= 0 or a region below 11 x 11): [n][channels * tiles][2] partials of
 * 32 x 32 tiles, added in a fixed order.  Refused with nothing launched: null pointers, n outside 1..65535, an unknown channel,
 * shave < 0, a region below 11 x 11, a row stride below 3 w. */
#define FSR_QUALITY_Y 0
#define FSR_QUALITY_RGB 1
size_t fsr_quality_u8_scratch(int n, int h, int w, int shave, int channel);
int fsr_quality_u8(const unsigned char* a, long long a_image_bytes, long long a_row_bytes, const unsigned char* b,
                   long long b_image_bytes, long long b_row_bytes, int n, int h, int w, int shave, int channel, float* out,
                   void* scratch, fsr_stream_t stream);

/* ------------------------------------------------------------------ AdamW (trainer.py:33-38, torch defaults)
 * One fused step over a flat float parameter arena: g' = g*grad_scale (1/world_size after a SUM all-reduce);
 * p *= 1 - lr*wd; m, v updated; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps).  `step_counter` is a DEVICE float
 * holding the number of steps taken so far: the update derives the bias corrections bc1 = 1 - beta1^t, bc2 = 1 - beta2^t
 * from t = step_counter + 1 and a one-thread launch behind it increments the counter (host-free, so a captured hipGraph replays).
 * Any float pointers are accepted; 16-byte aligned ones take 128-bit loads and stores. */
int fsr_adamw_step(float* p, const float* g, float* m, float* v, long long count, float lr, float beta1, float beta2,
                   float eps, float weight_decay, float* step_counter, float grad_scale, fsr_stream_t stream);

/* Dynamic loss scaling for the fp16 mode (no counterpart in the reference, which trains in fp32, trainer.py:33-43; the shape is
 * torch.cuda.amp.GradScaler's).  scale_state: DEVICE float[4] = {loss scale S, clean iterations, non-finite flag, skipped
 * iterations}; the backward passes are seeded with S (the caller reads scale_state[0] on the device).
 *   fsr_grad_nonfinite     raises the flag if any of the `count` gradients is inf / NaN (after the gradient all-reduce, so
 *                          every rank decides alike);
 *   fsr_adamw_step_scaled  fsr_adamw_step with g' = g*grad_scale/S -- and NO update at all (parameters, moments and step
 *                          counter untouched) while the flag is up;
 *   fsr_loss_scale_update  once per iteration, after the last optimizer step: flag up -> S *= backoff (>= 1), counters reset,
 *                          flag cleared; else after `growth_interval` clean iterations S *= growth.
 * All decisions are taken on the device: a captured hipGraph keeps adapting while it replays. */
int fsr_grad_nonfinite(const float* g, long long count, float* scale_state, fsr_stream_t stream);
int fsr_adamw_step_scaled(float* p, const float* g, float* m, float* v, long long count, float lr, float beta1, float beta2,
                          float eps, float weight_decay, float* step_counter, float grad_scale, const float* scale_state,
                          fsr_stream_t stream);
int fsr_loss_scale_update(float* scale_state, float growth_interval, float growth, float backoff, fsr_stream_t stream);

/* ------------------------------------------------------------------ AdamW with a device-side learning-rate schedule and a fused EMA
 * (added within ABI 16: a new entry point only).  fsr_adamw_step / fsr_adamw_step_scaled take the learning rate by value,
 * so a captured hipGraph replays the rate it was captured with.  Here the rate comes from `sched`, FSR_SCHED_WORDS floats in DEVICE
 * memory that the host writes when it installs a schedule:
 *   [0] kind: 0 constant, 1 multistep, 2 cosine     [1] base lr     [2] warm-up length W (0: none)     [3] cosine length T
 *   [4] min lr     [5] number of boundaries nb <= 8     [6] lr_used: the rate of the last update applied (written by one thread of the
 *   launch, never read by the update)     [7] clock e: updates applied since the schedule was installed
 *   [8..15] boundaries, ascending, as float step numbers     [16..24] nb + 1 lr values (the host computes base * gamma^k in double and
 *   casts; the device never takes a power for the schedule; slots behind nb / nb + 1 are not read).
 * Counters are floats (the clock as the step counter): exact up to 2^24 steps.
 * The update applied at clock e (the clock BEFORE it; torch's convention: the first update runs at f(0), milestone k takes effect for
 * update k + 1) uses
 *   constant / multistep:  val = values[#{boundaries <= e}]
 *   cosine:                val = min + 0.5 (base - min) (1 + cosf(pi fminf(e, T) / T))
 *   lr = e < W ? val ((e + 1) / W) : val
 * and is, with that lr, the same kernel as fsr_adamw_step (scale_state NULL: step counter and clock both advance by one) or
 * fsr_adamw_step_scaled (scale_state given: g' = g*grad_scale/S; while the non-finite flag is up NOTHING changes -- p, m, v, ema,
 * step counter, clock and lr_used stay bit-identical -- else step counter and clock advance by one): all three entry points launch
 * one kernel template, which differs only in where the rate comes from, so their results are equal bit for bit.
 * ema (nullable, `count` floats): after p' is computed, ema += (p' - ema) (1 - ema_decay), ema_decay in [0, 1). */
#define FSR_SCHED_WORDS 32
#define FSR_SCHED_KIND 0
#define FSR_SCHED_BASE 1
#define FSR_SCHED_WARMUP 2
#define FSR_SCHED_TOTAL 3
#define FSR_SCHED_MIN 4
#define FSR_SCHED_NB 5
#define FSR_SCHED_LR_USED 6
#define FSR_SCHED_CLOCK 7
#define FSR_SCHED_BOUNDS 8
#define FSR_SCHED_VALUES 16
#define FSR_SCHED_MAX_BOUNDARIES 8
int fsr_adamw_step_ex(float* p, const float* g, float* m, float* v, float* ema, long long count, float* sched, float beta1,
                      float beta2, float eps, float weight_decay, float* step_counter, float grad_scale, const float* scale_state,
                      float ema_decay, fsr_stream_t stream);

/* ------------------------------------------------------------------ crop + antialiased bicubic down-scale (dataloader.py:24-38)
 * For each of `n` samples: crop hr_size x hr_size at (crop_y[i], crop_x[i]) from the uint8 CHW image
 * image[i] (device pointers, heights/widths per image), hr = crop/127.5 - 1 (float NCHW [n,3,hr,hr]);
 * lr = antialiased bicubic (a = -0.5, support 2*scale) down-scale of the UNSCALED crop by `scale`,
 * then /127.5 - 1 (float NCHW [n,3,hr/scale,hr/scale]).  wtab: float [hr/scale][kmax] normalised
 * taps, xmin/xsize int [hr/scale] (identical for rows and columns; built on the host once). */
int fsr_crop_resize(const uint8_t* const* images, const int* img_h, const int* img_w, const int* crop_y,
                    const int* crop_x, int n, int hr_size, int scale, const float* wtab, const int* xmin,
                    const int* xsize, int kmax, float* hr_out, float* lr_out, float* tmp, fsr_stream_t stream);

/* ------------------------------------------------------------------ the eight symmetries of the rectangle (added within ABI 16: new entry
 * points only).  Code k in 0..7 acts on an H x W image in three steps: k & 1 flips the width axis, k & 2 flips the height
 * axis, then k & 4 transposes H and W -- codes 4..7 produce a W x H image.  The inverse of D_k is "transpose first, then the flips": as a
 * code, k itself except that 5 and 6 are each other's inverse.  Codes 0..3 and 4..7 are the two ORIENTATION GROUPS; one call serves
 * codes k0..k1 of one group.
 *
 * fsr_dihedral_members (self-ensemble input): src is n images [n,h,w,3], uint8 (src_is_u8 != 0) or float; out receives the float images
 * of members k0..k1, member-major: image (k - k0) n + i is D_k of image i, [h,w,3] for codes 0..3 and [w,h,3] for codes 4..7.  A uint8
 * source is mapped by fsr_u8_to_image's expression x / 127.5 - 1, so a member is D_k(fsr_u8_to_image(x)) bit for bit; a float source is
 * copied.
 *
 * fsr_dihedral_accumulate (self-ensemble output): y holds the float outputs of members k0..k1 in that layout, for a result of h x w
 * ([n,h,w,3] each for codes 0..3, [n,w,h,3] for 4..7).  They are read through the inverse transforms and added in code order, in float32,
 * onto the running sum: s = y_0 (k0 == 0; acc is not read) or acc (k0 > 0), then s = s + y_k' for the remaining codes of the call.  A
 * call with k1 < 7 stores s to acc [n,h,w,3]; the call with k1 == 7 stores to `out` instead: out_kind FSR_OUT_F32 float [n,h,w,3] =
 * 0.125f s (out may be acc), FSR_OUT_U8 uint8 [n,h,w,3] = (unsigned char)(clamp((0.125f s + 1) / 2, 0, 1) * 255), the truncating cast of
 * fsr_resample_image's FSR_OUT_U8 and of fsr_conv3x3's.  The order of the sum is that of the codes whatever the split into calls.
 *
 * fsr_crop_resize_aug (training augmentation): fsr_crop_resize with a per-sample code xform [n] (device ints; only the low 3 bits are
 * read): hr = D_k(crop) and lr = the down-scale of D_k(crop), pass 1 reading the source through D_k and everything behind it unchanged --
 * the batch fsr_crop_resize cuts from a data set holding D_k(image).  Crops are square, so every code keeps the shapes.
 *
 * Refused with nothing launched: null pointers, non-positive n, h, w, n > 65535, codes outside 0..7, k0 > k1, a range that spans both
 * groups, an unknown out_kind. */
int fsr_dihedral_members(const void* src, int src_is_u8, int n, int h, int w, int k0, int k1, float* out, fsr_stream_t stream);
int fsr_dihedral_accumulate(const float* y, int n, int h, int w, int k0, int k1, float* acc, void* out, int out_kind,
                            fsr_stream_t stream);
int fsr_crop_resize_aug(const uint8_t* const* images, const int* img_h, const int* img_w, const int* crop_y, const int* crop_x,
                        const int* xform, int n, int hr_size, int scale, const float* wtab, const int* xmin, const int* xsize, int kmax,
                        float* hr_out, float* lr_out, float* tmp, fsr_stream_t stream);

/* ------------------------------------------------------------------ training degradations (added within ABI 16: new entry points only)
 * Both work on float NCHW batches [n,3,h,w] in [-1,1] (what fsr_crop_resize writes); every per-sample array is a DEVICE pointer.
 *
 * fsr_degrade_blur_noise: separable Gaussian blur (horizontal pass in -> tmp, vertical pass tmp -> out), then additive noise in the
 * vertical pass's epilogue: two launches.  taps: float [n][FSR_BLUR_TAPS], sample i uses taps[i][0 .. 2 radii[i]] for the offsets
 * j = -radii[i] .. radii[i] (built and normalised on the host), float accumulation in that order, source index clamped at the borders;
 * radii[i] = 0 copies the sample (radii above FSR_BLUR_MAX_RADIUS are read as that).  noise_sigma: float [n] in 8-bit code units, 0 =
 * none; element e = (c h + y) w + x of sample i gets x += z * noise_sigma[i] * (2 / 255) with z = sqrtf(-2 logf(U1)) cosf(6.2831855f U2),
 * U1 = ((a >> 8) + 1) 2^-24, U2 = (b >> 8) 2^-24, a = mix32(mix32(s0 + 2e) ^ s1), b = mix32(mix32(s0 + 2e + 1) ^ s1), (s0, s1) =
 * seeds[2i], seeds[2i + 1], mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 * taps = radii = NULL: the noise-only form, one launch in -> out (tmp unused, may be NULL).  noise_sigma = seeds = NULL: blur only.
 * in == out is allowed; tmp must be a third buffer of the same size.
 *
 * fsr_jpeg_roundtrip: what a baseline JPEG encode + decode at quality[i] (int [n], 1..100, libjpeg's scaling of the Annex K tables;
 * 0 copies the sample, values above 100 are read as 100) does to sample i, without the entropy coder: one launch, one workgroup per
 * 16x16 pixels.  subsampling: FSR_CHROMA_420 (2x2 chroma mean, replicated back) or FSR_CHROMA_444.  The input code (x + 1) 127.5 is
 * clamped to [0, 255] but NOT rounded; the output is clamp(rint(.), 0, 255) / 127.5 - 1.
 * Refused (-1 / -2, nothing launched): null pointers, n, h or w < 1, 3 h w >= 2^31, an unknown subsampling. */
#define FSR_BLUR_MAX_RADIUS 9
#define FSR_BLUR_TAPS 19
int fsr_degrade_blur_noise(const float* in, float* out, float* tmp, int n, int h, int w, const float* taps, const int* radii,
                           const float* noise_sigma, const unsigned* seeds, fsr_stream_t stream);
int fsr_jpeg_roundtrip(const float* in, float* out, int n, int h, int w, const int* quality, int subsampling, fsr_stream_t stream);

/* ------------------------------------------------------------------ per-sample 2-D filter (added within ABI 16: a new entry point only)
 * fsr_filter2d: a non-separable K x K filter per sample on a float NCHW batch [n,3,h,w], K = 2 r + 1 <= 21: the blur of a kernel bank
 * (rotated / generalised / plateau Gaussians, sinc) in front of a sampler.  One launch:
 *   out[i][c][y][x] = sum_{dy = -r..r} sum_{dx = -r..r} taps[i][(dy + r) K + dx + r] * in[i][c][clamp(y + dy)][clamp(x + dx)]
 * -- correlation, not convolution; the source index is clamped at the borders; float accumulation from 0 in the order dy outer, dx inner.
 * taps: DEVICE float [n][FSR_FILTER2D_TAPS], sample i's K x K taps row-major and packed at the start of its block (built and normalised
 * on the host; the slots behind K * K are not read).  radii: DEVICE int [n], read as clamped to 0 .. FSR_FILTER2D_MAX_RADIUS;
 * radii[i] = 0 copies the sample bit for bit through the same launch (its taps are not read).  One workgroup owns
 * FSR_FILTER2D_TILE_H x FSR_FILTER2D_TILE_W outputs of one (sample, channel).
 * Refused (-1 / -2, nothing launched): null pointers, n, h or w < 1, in == out, 3 h w >= 2^31. */
#define FSR_FILTER2D_MAX_RADIUS 10
#define FSR_FILTER2D_TAPS 441
#define FSR_FILTER2D_TILE_H 32
#define FSR_FILTER2D_TILE_W 64
int fsr_filter2d(const float* in, float* out, int n, int h, int w, const float* taps, const int* radii, fsr_stream_t stream);

/* fsr_resize_select: separable down-scale (or any resize) of a float NCHW batch [n,3,ih,iw] -> [n,3,oh,ow] with a tap table chosen per
 * sample, horizontal pass in -> tmp [n,3,ih,ow], then vertical pass tmp -> out: two launches, float accumulation in tap order.
 *   tmp[i][c][y][xo]  = sum_{k < xsize[f][xo]} wx[f][xo][k] * in[i][c][y][xmin[f][xo] + k]
 *   out[i][c][yo][xo] = sum_{k < ysize[f][yo]} wy[f][yo][k] * tmp[i][c][ymin[f][yo] + k][xo]            f = sel[i]
 * wx float [nf][ow][kx], xmin / xsize int [nf][ow] and wy float [nf][oh][ky], ymin / ysize int [nf][oh]: nf normalised tables per axis in
 * the layout of fsr_crop_resize's (the caller keeps xmin + xsize <= iw, xsize <= kx and likewise for y); sel: int [n], read as clamped
 * to 0 .. nf - 1.  Every array is a DEVICE pointer.  No [-1,1] mapping: float in, float out.
 * Refused (-1 / -2, nothing launched): null pointers, extents, nf, kx or ky < 1, tmp == in or out, in == out, 3 ih iw >= 2^31. */
int fsr_resize_select(const float* in, float* out, float* tmp, int n, int ih, int iw, int oh, int ow, const float* wx, const int* xmin,
                      const int* xsize, int kx, const float* wy, const int* ymin, const int* ysize, int ky, int nf, const int* sel,
                      fsr_stream_t stream);

/* fsr_degrade_noise_kinds: fsr_degrade_blur_noise's noise-only form with a kind per sample.  strength: float [n], flags: int [n] of
 * FSR_NOISE_SHOT | FSR_NOISE_GREY, seeds as there.  Without FSR_NOISE_SHOT strength is the sigma of fsr_degrade_blur_noise and the
 * result is that call's, bit for bit.  FSR_NOISE_SHOT: strength is a gain g in code units and
 *   x += z * sqrtf(g * v) * (2 / 255),   v = clamp((x + 1) * 127.5, 0, 255)
 * -- the normal approximation of Poisson (shot) noise, not a Poisson sampler.  FSR_NOISE_GREY: the hash's element index is y w + x
 * in place of (c h + y) w + x, so the three channels of a pixel share one z.  strength <= 0 copies the sample.  One launch. */
enum { FSR_NOISE_SHOT = 1, FSR_NOISE_GREY = 2 };
int fsr_degrade_noise_kinds(const float* in, float* out, int n, int h, int w, const float* strength, const int* flags, const unsigned* seeds,
                            fsr_stream_t stream);

/* ------------------------------------------------------------------ strided element-wise losses (added within ABI 16: new entry points only)
 * The pixel term of the training objective and the least-squares adversarial term.  a, b: float [n,c,h,w], each read through its OWN
 * four strides (in elements; an NCHW view of an NHWC buffer, a planar batch, a slice) -- nothing is copied.  With d = a - b and
 * count = n c h w:   loss[0] = sum psi(d) / count,   da = gscale[0] / count * psi'(d)   (gscale: device scalar, the upstream gradient;
 * da is written through a's strides; b is the target and gets no gradient).
 *   FSR_LOSS_L1           psi = |d|                   psi' = sign(d), 0 at d = 0
 *   FSR_LOSS_SMOOTH_L1    fsr_smooth_l1_fwd / _bwd's expressions (beta 1)
 *   FSR_LOSS_CHARBONNIER  psi = sqrt(d d + eps eps)   psi' = d / sqrt(d d + eps eps)        param = eps (positive, finite)
 *   FSR_LOSS_MSE          psi = d d                   psi' = 2 d
 * param is ignored by the other kinds.  The forward is one streaming launch (lanes = pixels, the channel loop inside the thread) plus
 * the order-fixed second-level sum of at most 1024 workgroup partials in `scratch` (fsr_elem_loss_scratch() bytes): no float atomics.
 * Refused with nothing launched: null pointers, non-positive extents, n c h w >= 2^31, an unknown kind, a Charbonnier eps that is not
 * positive and finite, and -- over the axes longer than 1 -- negative, zero or overlapping strides of either operand. */
enum { FSR_LOSS_L1 = 0, FSR_LOSS_SMOOTH_L1 = 1, FSR_LOSS_CHARBONNIER = 2, FSR_LOSS_MSE = 3 };
size_t fsr_elem_loss_scratch(void);
int fsr_elem_loss_fwd(int kind, float param, const float* a, long long sa_n, long long sa_c, long long sa_h, long long sa_w,
                      const float* b, long long sb_n, long long sb_c, long long sb_h, long long sb_w, int n, int c, int h, int w,
                      float* loss, void* scratch, fsr_stream_t stream);
int fsr_elem_loss_bwd(int kind, float param, const float* a, long long sa_n, long long sa_c, long long sa_h, long long sa_w,
                      const float* b, long long sb_n, long long sb_c, long long sb_h, long long sb_w, const float* gscale, float* da,
                      int n, int c, int h, int w, fsr_stream_t stream);

/* ------------------------------------------------------------------ strided row-block copy (ABI 15; the banded tail)
 * A frame of H2 rows is covered by nwin = ceil(H2 / R) windows of Hw >= R + 4 rows: window k owns the core rows
 * [k R, min((k + 1) R, H2)) and starts at row s_k = clamp(k R - 2, 0, H2 - Hw).  The windows of all images are numbered
 * f = image * nwin + k; one call moves the windows f = first .. first + count - 1 (count <= 65535), window f being image f - first
 * of the group buffer:
 *   scatter = 0 (gather): rows [s_k, s_k + Hw) of image f / nwin of `src` -> rows [0, Hw) of group image f - first of `dst`;
 *   scatter = 1: rows [(k R - s_k) mul, (core_hi - s_k) mul) of group image f - first of `src` -> rows [k R mul, core_hi mul) of
 *                image f / nwin of `dst` (mul: rows of this tensor per row the windows are counted in).
 * Rows are row_bytes bytes, back to back inside an image; consecutive images lie src_pitch / dst_pitch bytes apart (a plane of a
 * planar payload: bases at the plane, pitches of the payload).  All offsets are 64-bit.  16-byte accesses when both bases, both
 * pitches and row_bytes are multiples of 16, else 4-byte, else single bytes (fsr_last_kernel() names the width).  The caller
 * vouches for the extents of both buffers; null pointers, non-positive extents, R < 1, Hw > H2 and Hw < R + 4 are refused. */
int fsr_copy_rows(const void* src, long long src_pitch, void* dst, long long dst_pitch, long long row_bytes, int first, int count,
                  int H2, int Hw, int R, int mul, int scatter, fsr_stream_t stream);

/* ------------------------------------------------------------------ PNG -> .npy ingest (host code, no device work)
 * train.py:22-37 of the reference converts the data set once: PIL decode -> RGB -> uint8 CHW -> np.save, on 16 Python threads.
 * fsr_png_to_npy does the same natively on `threads` threads (zlib inflate, the five PNG row filters, grey / palette / alpha
 * handled as PIL's convert("RGB") does: replicated / looked up / dropped), writing .npy format 1.0 ('|u1', C order, (3, H, W)).
 * status[i] (optional): 0 converted; -1 not a PNG; -2 corrupt; -3 I/O error; -4 a PNG this decoder does not take (interlaced,
 * 16-bit, grey below 8 bits) -- the caller decodes exactly those files its own way.  Returns the number of files NOT converted.
 * fsr_png_decode_chw decodes one file into `out_chw` (3 * H * W bytes; null: only report the size). */
int fsr_png_to_npy(const char* const* png_paths, const char* const* npy_paths, int count, int threads, int* status);
int fsr_png_decode_chw(const char* png_path, unsigned char* out_chw, size_t capacity, int* height, int* width);

#ifdef __cplusplus
}
#endif
#endif /* FSR_HIP_H */
