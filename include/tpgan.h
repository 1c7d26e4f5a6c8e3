/*
 * tpgan.h — C-ABI of libtpgan_hip.so, the MI355X (gfx950) kernels of the TP-GAN
 * generator/discriminator hot path.
 *
 * The reference (PandaKenWei/TP-GAN) has no FFI: its hot path is torch.nn layers called
 * from Python.  Each entry point below replaces one aten call the
 * reference's layer factories make; the Python host side (tp-gan_amd/tpgan_lib.py) binds
 * them with ctypes and keeps the reference's module/class/state_dict API on top.
 *
 *   tpg_conv2d_fwd          nn.Conv2d / nn.ConvTranspose2d forward + bias + activation
 *                           (+ residual add) — ModificationLayer.py:54-123 conv(),
 *                           :158-202 deconv(), :298-302 ResidualBlock.forward,
 *                           and the ReflectionPad2d of :83-96 (pad_mode = reflect);
 *                           also Linear (fc1, D_and_G_model.py:212) as a full-kernel conv.
 *   tpg_conv2d_bwd_data     the input gradient of the same op (aten convolution_backward)
 *   tpg_conv2d_bwd_filter   the weight gradient (accumulated into fp32)
 *   tpg_act_bwd             activation' mask (LeakyReLU 0.01 / ReLU, from the saved output)
 *                           + bias gradient
 *   tpg_fold_taps           im2col-lite for the 3-channel convs (taps folded into channels)
 *   tpg_copy4d              dtype/layout conversion and torch.cat into a channel slice
 *                           (D_and_G_model.py:100,102,104,293,298,307,311,312,317,318,323,324)
 *   tpg_local_fuse_fwd/bwd  LocalFuser (D_and_G_model.py:132-159): zero-pad + max over 4 parts
 *   tpg_maxout2_fwd/bwd     fc2 maxout, MaxPool1d(2,2) (D_and_G_model.py:214,290)
 *   tpg_adam                the optimizer update (UtilityMethods.py:14-41 getOptimizer 'Adam')
 *   tpg_dwconv2d_*          depthwise 3x3 conv of MobileNetV2's inverted residuals (MobileNetV2.py:105)
 *   tpg_maxpool2d_*         ResNet stem MaxPool2d(3, 2, 1) (ResNet.py:33)
 *   tpg_avgpool_*           AdaptiveAvgPool2d(1) (MobileNetV2.py:173, ResNet.py:45)
 *   tpg_bn_fold             eval-mode BatchNorm2d folded into conv weights (MobileNetV2.py:100-112)
 *   tpg_bn_train_fwd/bwd    training-mode BatchNorm2d (+ fused activation) with running statistics
 *   tpg_landmark_boxes      get_5_landmarks_pixal_position (UtilityMethods.py:148-164) + the crop
 *                           boxes of DataAndDataset.process (DataAndDataset.py:42-54)
 *   tpg_crop_normalize      PIL crop + ToTensor + x*2-1 (DataAndDataset.py:51-54,216-220,252-255)
 *   tpg_resize_u8           Image.resize(size, Image.LANCZOS) of RGB u8 images of different sizes,
 *                           bit for bit (DataAndDataset.py:247-251); tpg_resize_coeffs and
 *                           tpg_resize_pack_job build its tables and job records on the host
 *   tpg_similarity_fit      least-squares similarity transform from a template of face points to each
 *                           face's detected points, and tpg_affine_warp_u8, the photo resampled
 *                           through it into the generator's frame (build-defined, no reference code:
 *                           the reference's TestDataset only takes tight, upright face crops);
 *                           tpg_warp_pack_job builds the warp's job records on the host
 *   tpg_denorm_u8           the generator's [-1, 1] output back to u8 HWC pixels: ToPILImage /
 *                           torchvision.utils.save_image's rounding of (x+1)/2 (the reference has no
 *                           inference script; its training loop would save samples that way)
 *   tpg_image_metrics_u8    per-image squared error (PSNR) and SSIM of a u8 result against the u8
 *                           ground truth (build-defined, no reference code: the validation pass of
 *                           a TP-GAN training loop, as Pretrain.py:197-249 is for the landmark net)
 *   tpg_l2_normalize        unit-length f32 embeddings of the identity extractor's features
 *                           (torch.nn.functional.normalize; build-defined like the two below: the
 *                           reference has no evaluation script, TP-GAN is judged on rank-1
 *                           identification and identity-feature similarity)
 *   tpg_cosine_topk         the k best gallery rows of every probe by cosine similarity, without
 *                           the P x G matrix (torch.matmul + torch.topk); tpg_cosine_topk_workspace
 *                           sizes its scratch
 *   tpg_cosine_pairs        row-wise cosine similarity of two feature batches
 *                           (torch.nn.functional.cosine_similarity)
 *
 * Conventions
 *   - Every tensor is described by tpg_tensor: a device pointer, a dtype and the element
 *     strides of its LOGICAL NCHW view (n, c, h, w).  Kernels are fastest on
 *     channels-last (NHWC) tensors whose pixel stride is a multiple of 8 elements, which
 *     is what the host side allocates; any other strides are accepted on slower paths.
 *   - Weights are the fp32 master parameters, logical [a][b][kh][kw]
 *     (Conv2d: a = out, b = in; ConvTranspose2d: a = in, b = out), any strides.
 *   - Ownership: every pointer is caller-owned device memory; the library never
 *     allocates or frees and keeps no state besides a thread-local error string.
 *   - Work space: query tpg_conv2d_workspace(); pass at least that many bytes.
 *   - Streams: every call enqueues on the given stream only, never synchronises, and is
 *     therefore legal inside hipStreamBeginCapture (hipGraph) regions.
 *   - Errors: 0 on success, negative for a bad descriptor / unsupported shape, positive
 *     hipError_t for a launch failure; tpg_last_error() returns the message.
 */
#ifndef TPGAN_H
#define TPGAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* tpg_stream_t; /* hipStream_t */

enum { TPG_F32 = 0, TPG_BF16 = 1, TPG_F16 = 2 };
enum { TPG_ACT_NONE = 0, TPG_ACT_RELU = 1, TPG_ACT_LEAKY = 2, TPG_ACT_RELU6 = 3 };
enum { TPG_PAD_ZERO = 0, TPG_PAD_REFLECT = 1 };
enum { TPG_OP_FWD = 0, TPG_OP_BWD_DATA = 1, TPG_OP_BWD_FILTER = 2 };

typedef struct tpg_tensor {
  void* data;
  int32_t dtype;      /* TPG_F32 / TPG_BF16 / TPG_F16 */
  int32_t reserved;
  int64_t stride[4];  /* element strides of the logical (n, c, h, w) view */
} tpg_tensor;

typedef struct tpg_conv_desc {
  int32_t n;                      /* batch */
  int32_t in_c, in_h, in_w;       /* input  (logical NCHW) */
  int32_t out_c, out_h, out_w;    /* output (logical NCHW) */
  int32_t kh, kw;                 /* kernel */
  int32_t stride_h, stride_w;
  int32_t pad_t, pad_b, pad_l, pad_r;
  int32_t pad_mode;               /* TPG_PAD_*; reflect only for transposed == 0 */
  int32_t transposed;             /* 0: Conv2d, 1: ConvTranspose2d (output_padding = out - natural) */
  int32_t dtype;                  /* activation / arithmetic dtype: TPG_F32 (exact fp32 MFMA), TPG_BF16 or
                                     TPG_F16 (16-bit MFMA operands, fp32 accumulate) */
  int32_t act;                    /* TPG_ACT_* applied after bias (+ residual) */
  float slope;                    /* LeakyReLU negative slope */
  float res_scale;                /* ResidualBlock scaling_factor (ModificationLayer.py:300) */
  int32_t ksplit;                 /* 0 = automatic; >= 1 forces the K split (bwd_filter: pixel splits) */
  int32_t algo;                   /* 0 = automatic; bwd_filter: 1..5 = tile 256x128, 128x128, 128x64,
                                     64x128, 64x64 (used with ksplit >= 1; autotuners set both);
                                     6..9 = kernel-row halo kernel, tile 128x64, 128x32, 64x64,
                                     64x32 (stride-1 bf16 Conv2d, 3/5/7-wide kernels, output
                                     width a multiple of 64); 10, 11 = image-halo kernel, tile
                                     128x32, 64x32 (2x2 / 3x3 kernels, output width 8/16/32/64·m,
                                     64 / width dividing the height); 12 = kernel-row halo kernel,
                                     tile 256x32 (one a-tile up to 256 output channels: dY read
                                     once per b-tile); 13 = kernel-row halo kernel, dense tile
                                     80 x (7 taps x 80): one block per kernel row of a 7-wide
                                     kernel with at most 80 channels on each side, a tap per
                                     wave (16-bit, output width a multiple of 64; no dead-block
                                     skip); 14 = kernel-row halo kernel, dense five-tap tile: one
                                     block per kernel row of a 5-wide kernel and per (a, b) tile of
                                     at most 112 x 112 channels, the 5 x (b / 16) column blocks
                                     dealt to the 8 waves (16-bit, output width a multiple of 64;
                                     no dead-block skip); -30 when not covered */
  int32_t flags;                  /* TPG_FLAG_*: WPACKED = w.data is the image tpg_conv2d_pack_jobs /
                                     tpg_pack_run produced for this descriptor and op */
  int32_t data_ksplit;            /* 0 = automatic; >= 1 forces the k-step split of the forward and
                                     input-gradient launches (1: no split, so no split-K finish
                                     launch); set by autotuners; ignored in deterministic mode */
  int32_t data_algo;              /* forward / input-gradient kernel of small-map convs with several
                                     taps: 0 = planner's rule, 1 = the halo-tiled kernel, 2 = the
                                     tap-DMA pointwise kernel where eligible (16-bit, channels a
                                     multiple of 32); set by autotuners */
  int32_t in_act;                 /* tpg_conv2d_bwd only: TPG_ACT_* of the layer that PRODUCED x (x = that
                                     layer's activated output, saved by this op's forward): the input
                                     gradient leaves the launch as dx * in_act'(x) -- the producer's
                                     activation backward, applied in this launch's epilogue (after a
                                     DX_ACCUM add), so the producer's own backward takes it as its
                                     already-masked g.  0 (TPG_ACT_NONE) everywhere else */
  float in_slope;                 /* LeakyReLU negative slope of in_act */
} tpg_conv_desc;

enum { TPG_FLAG_WPACKED = 1, TPG_FLAG_CONCURRENT = 2, TPG_FLAG_DX_ACCUM = 4 };
/* CONCURRENT: the op runs beside other streams' work (plan grids for a quarter of the chip:
   fewer splits).  DX_ACCUM (tpg_conv2d_bwd_data / tpg_conv2d_bwd): dx holds another gradient
   contribution of the same input on entry and the input-gradient launch adds it in its
   epilogue (dx = dgrad + dx; e.g. a residual block's shortcut gradient), instead of a
   separate add; zero-padded, non-GEMM-form geometries only (-32 otherwise). */

/* Workspace bytes needed by op (TPG_OP_*) for this descriptor. */
size_t tpg_conv2d_workspace(const tpg_conv_desc* d, int32_t op);

/* Pre-packed weights (fwd and bwd_data convert the fp32 master weight into the kernels'
 * tile order on every call unless desc.flags has TPG_FLAG_WPACKED):
 *   tpg_conv2d_packed_bytes  bytes of the packed image of (d, op), op = FWD or BWD_DATA
 *   tpg_conv2d_pack_jobs     describe packing w into wp as <= max_jobs opaque jobs of
 *                            tpg_pack_job_bytes() each, written to host memory `jobs`;
 *                            returns the job count (negative on error)
 *   tpg_pack_prepare         lay a host job array out for one launch; returns its block count
 *   tpg_pack_run             run n prepared jobs (copied to device memory) in ONE launch
 * The image assumes 16-byte aligned channels-last activations (and dense NHWC for the
 * full-kernel GEMM forms); a call whose tensors need another plan returns -21. */
size_t tpg_conv2d_packed_bytes(const tpg_conv_desc* d, int32_t op);
size_t tpg_pack_job_bytes(void);
int32_t tpg_conv2d_pack_jobs(const tpg_conv_desc* d, int32_t op, tpg_tensor w, void* wp, void* jobs,
                             int32_t max_jobs);
int64_t tpg_pack_prepare(void* jobs, int32_t n);
int32_t tpg_pack_run(const void* jobs_dev, int32_t n, int64_t nblocks, tpg_stream_t stream);

/* y = act(conv(x, w) + bias [+ res_scale * residual]).  residual.data may be NULL; bias may be NULL. */
int32_t tpg_conv2d_fwd(const tpg_conv_desc* d, tpg_tensor x, tpg_tensor w, const float* bias,
                       tpg_tensor residual, tpg_tensor y, void* ws, size_t ws_bytes, tpg_stream_t stream);

/* dx = dconv/dx applied to g (g is the already-masked output gradient, see tpg_act_bwd). */
int32_t tpg_conv2d_bwd_data(const tpg_conv_desc* d, tpg_tensor g, tpg_tensor w, tpg_tensor dx,
                            void* ws, size_t ws_bytes, tpg_stream_t stream);

/* dw += dconv/dw (fp32, dw strides given by the tensor; dw.dtype must be TPG_F32). */
int32_t tpg_conv2d_bwd_filter(const tpg_conv_desc* d, tpg_tensor x, tpg_tensor g, tpg_tensor dw,
                              void* ws, size_t ws_bytes, tpg_stream_t stream);

/* The plan tpg_conv2d_bwd_filter (and step 3 of tpg_conv2d_bwd) runs for these tensors: host
 * arithmetic on the descriptor, dtypes, strides and pointer alignment only -- no device work,
 * nothing dereferenced, nothing launched or flushed.  Returns what tpg_conv2d_bwd_filter would
 * return before its first launch (0, or e.g. -30 for a desc.algo that does not cover the shape;
 * *out is then untouched).  Reads the same process state as the launch: desc.flags CONCURRENT,
 * tpg_set_deterministic. */
enum { TPG_WGRAD_GENERIC = 0, TPG_WGRAD_FLAT = 1, TPG_WGRAD_ROW_HALO = 2, TPG_WGRAD_IMAGE_HALO = 3 };
enum {
  TPG_WGRAD_SUMS_BIAS = 1, /* the launch adds the bias gradient when given one (tpg_conv2d_bwd) */
  TPG_WGRAD_BFLAT = 2,     /* flat kernel: columns flattened over taps */
  TPG_WGRAD_FASTP = 4,     /* flat kernel: division-free addressing of the pixel-grid operand */
  TPG_WGRAD_FASTQ = 8,     /* flat kernel: the same for the gathered operand */
  TPG_WGRAD_SKIP = 16,     /* halo kernels: MFMAs of all-padding blocks of edge tiles skipped */
  TPG_WGRAD_GROUPED = 32   /* recorded, not launched, inside a launch group (tpg_group_begin) */
};
typedef struct tpg_wgrad_plan {
  int32_t kernel;          /* TPG_WGRAD_*: generic (tpg_wgrad.hip), flat DMA (tpg_wgrad2.hip), kernel-row
                              halo or image halo (tpg_wgrad_rh.hip) */
  int32_t cfg;             /* the kernel family's own tile index */
  int32_t tile_m, tile_n;  /* tile: a channels x b columns */
  int32_t splits;          /* pixel splits (1: every dW element added once) */
  int32_t per_split;       /* pixels per split (generic, flat) or 64-pixel k-tiles per split (halo) */
  int32_t tiles;           /* output tiles; the grid is tiles x splits blocks */
  int32_t taps_per_block;  /* halo kernels: kernel rows x taps one block accumulates; else 0 */
  int32_t bias_share;      /* column tiles the bias sums are spread over (0: generic kernel) */
  int32_t flags;           /* TPG_WGRAD_SUMS_BIAS | ... */
} tpg_wgrad_plan;
int32_t tpg_conv2d_wgrad_plan(const tpg_conv_desc* d, tpg_tensor x, tpg_tensor g, tpg_tensor dw,
                              tpg_wgrad_plan* out);

/* The plan tpg_conv2d_fwd (op TPG_OP_FWD: a = x, y = y), tpg_conv2d_bwd_data (TPG_OP_BWD_DATA:
 * a = g, y = dx) or the masked input-gradient mode of tpg_conv2d_bwd (TPG_OP_BWD_DATA_MASKED:
 * a = gy, y = dx, m = the forward's saved output, g = the buffer g is written to) runs for these
 * tensors and a workspace of ws_bytes, under the same rules as tpg_conv2d_wgrad_plan: host
 * arithmetic only, nothing dereferenced, launched or flushed.  x (input gradients with
 * desc.in_act only; else ignored) is the conv's input.  The weights are taken as valid (fp32, or
 * the packed image when desc.flags has WPACKED) and the forward as having no residual.  Returns
 * the status the launch would give (0, -4, -20, -21, -32; -31: the call has no masked mode and
 * tpg_conv2d_bwd takes the separate activation pass) and leaves *out alone when it is not 0. */
enum { TPG_OP_BWD_DATA_MASKED = 3 };
enum { TPG_DATA_GENERIC = 0, TPG_DATA_HALO = 1, TPG_DATA_POINTWISE = 2 };
enum {
  TPG_DATA_COMPOSITE = 1,    /* full-kernel GEMM form over flattened (y, x, c) channels */
  TPG_DATA_DILATED = 2,      /* strided sub-pixel classes run as one zero-insertion problem */
  TPG_DATA_REFLECT_FOLD = 4, /* gradient of the reflect-padded input into a temp, folded onto dx */
  TPG_DATA_MASKED = 8,       /* act'(m) applied while the halo is staged; g written on the way */
  TPG_DATA_IN_ACT = 16       /* desc.in_act applied by the epilogues (else a separate pass) */
};
#define TPG_DATA_MAX_PROBS 16 /* a stride-4 ConvTranspose2d has 16 sub-pixel classes */
typedef struct tpg_data_prob {
  int32_t kernel;             /* TPG_DATA_*: generic implicit GEMM (tpg_igemm.hip), halo (tpg_halo.hip) or
                                 pointwise (tpg_pw.hip), after every fallback */
  int32_t cfg;                /* the generic or halo kernel's config id */
  int32_t th, tw, img;        /* halo plan: sub-tile and sub-tiles per block (generic: 0) */
  int32_t bn, rows;           /* output channels and rows of a block */
  int32_t halo_px;            /* halo pixels per LDS buffer (generic: 0) */
  int32_t taps;
  int32_t ksteps;             /* k-steps (halo: 64-byte channel steps per tap; generic: k-tiles) */
  int32_t ksplit, kps;        /* splits over k-steps and steps per split */
  int32_t paired;             /* halo: the last k-step runs two taps per MFMA */
  int32_t pw_tile;            /* pointwise kernel: tile 1..4 (128x128, 128x64, 64x128, 64x64); else 0 */
  uint64_t wp_off, wp_bytes;  /* weight region, in the workspace or (WPACKED) the packed image */
  uint64_t sk_bytes;          /* fp32 split-K slices at sk_off (0: none) */
} tpg_data_prob;
typedef struct tpg_data_plan {
  int32_t nprobs;
  int32_t flags;              /* TPG_DATA_COMPOSITE | ... */
  uint64_t ws_bytes;          /* tpg_conv2d_workspace(d, op) */
  uint64_t packed_bytes;      /* the plan's weight regions (dense tensors: tpg_conv2d_packed_bytes(d, op)) */
  uint64_t tmp_bytes;         /* reflect fold: temp at the start of the workspace */
  uint64_t sk_off;            /* workspace offset of the split-K slices the problems share */
  tpg_data_prob prob[TPG_DATA_MAX_PROBS];
} tpg_data_plan;
int32_t tpg_conv2d_data_plan(const tpg_conv_desc* d, int32_t op, tpg_tensor a, tpg_tensor y, tpg_tensor m,
                             tpg_tensor g, tpg_tensor x, size_t ws_bytes, tpg_data_plan* out);

/* Fused per-layer backward of tpg_conv2d_fwd's op (replaces aten convolution_backward of the
 * nn.Conv2d / nn.ConvTranspose2d built at ModificationLayer.py:101 / :186, plus the activation
 * backward of the layer's LeakyReLU / ReLU):
 *   g  = gy * act'(y)          (y = the forward's saved output; written to g — with
 *                               TPG_ACT_NONE g is gy itself and g may be empty)
 *   dx = input gradient of g   (dx.data NULL: skipped)
 *   dw += weight gradient      (dw.data NULL: skipped; desc.algo / ksplit as tpg_conv2d_bwd_filter)
 *   dbias += sum of g          (NULL: skipped)
 * For a stride-1 "same" zero-padded Conv2d the activation' is applied while the input
 * gradient's halo is staged (the input-gradient launch writes g as it goes) and the bias sum
 * rides on the weight-gradient launch (one MFMA against ones per fragment); other layers run
 * tpg_act_bwd first.  w may be a pre-packed image (desc.flags WPACKED, bwd_data layout).
 * g must have y's strides for the fused form.  desc.in_act != NONE: dx = (input gradient
 * [+ dx's DX_ACCUM entry values]) * in_act'(x), fused into the input-gradient epilogue where x
 * has dx's strides (an in-place pass over dx otherwise); needs x and dx. */
int32_t tpg_conv2d_bwd(const tpg_conv_desc* d, tpg_tensor x, tpg_tensor w, tpg_tensor y, tpg_tensor gy,
                       tpg_tensor g, tpg_tensor dx, tpg_tensor dw, float* dbias, void* ws, size_t ws_bytes,
                       tpg_stream_t stream);

/* Launch groups (the four LocalPathways of D_and_G_model.py:18-110 run layer by layer in
 * lockstep, replacing four per-patch launches per op with one).  Between begin and end, the
 * calling thread's conv / activation-backward calls record their kernels instead of launching
 * them; tpg_group_member() opens the next member (one independent problem, e.g. one patch's
 * tpg_conv2d_fwd or tpg_conv2d_bwd).  tpg_group_end() launches the record: where every member
 * issued the same kernel sequence, one grid per position covers all members, otherwise the
 * launches run one by one in call order.  A call that needs another kernel flushes the record
 * first, so the semantics are always those of the calls run in order.  Tensors and workspaces
 * of the recorded calls must stay allocated until tpg_group_end returns. */
void tpg_group_begin(void);
void tpg_group_member(void);
int32_t tpg_group_end(void);

/* g = gy * act'(y) over logical [n, c, h, w]; dbias[c] += sum g (dbias may be NULL). */
int32_t tpg_act_bwd(int32_t n, int32_t c, int32_t h, int32_t w, int32_t act, float slope,
                    tpg_tensor gy, tpg_tensor y, tpg_tensor g, float* dbias, tpg_stream_t stream);

/* out = in over logical [n, c, h, w] with dtype conversion; in and out may have any strides
 * (an out view offset into a wider channels-last buffer implements torch.cat). */
int32_t tpg_copy4d(int32_t n, int32_t c, int32_t h, int32_t w, tpg_tensor in, tpg_tensor out,
                   tpg_stream_t stream);

/* Tap folding for thin-input convs (3-channel images): y[n][(fy*fw + fx)*c + ci][y'][x'] =
 * x[n][ci][y'*sh + fy - pt][x'*sw + fx - pl] (zero outside), y logical [n, fh*fw*c, oh, ow];
 * the conv on y with the weight viewed as [out][fh*fw*c][kh/fh][kw/fw] equals the original
 * (ModificationLayer.py:54-123 conv() on the RGB inputs of D_and_G_model.py:33,193,415).
 * backward != 0: x (as dx) = the sum over every folded copy of y (as the incoming gradient). */
int32_t tpg_fold_taps(int32_t n, int32_t c, int32_t h, int32_t w, int32_t fh, int32_t fw, int32_t sh, int32_t sw,
                      int32_t pt, int32_t pl, int32_t oh, int32_t ow, tpg_tensor x, tpg_tensor y, int32_t backward,
                      tpg_stream_t stream);

/* LocalFuser: part k (logical [n, c, ph[k], pw[k]]) is placed at (top[k], left[k]) of an
 * out_h x out_w zero canvas; y = max over k, argmax = first k attaining it (uint8, NHWC order). */
int32_t tpg_local_fuse_fwd(int32_t n, int32_t c, int32_t out_h, int32_t out_w, const tpg_tensor* parts,
                           const int32_t* ph, const int32_t* pw, const int32_t* top, const int32_t* left,
                           tpg_tensor y, uint8_t* argmax, tpg_stream_t stream);
int32_t tpg_local_fuse_bwd(int32_t n, int32_t c, int32_t out_h, int32_t out_w, tpg_tensor gy,
                           const uint8_t* argmax, const tpg_tensor* dparts, const int32_t* ph,
                           const int32_t* pw, const int32_t* top, const int32_t* left, tpg_stream_t stream);

/* fc2 maxout: y[b, j] = max(x[b, 2j], x[b, 2j+1]) (first index wins ties), x logical [b, 2m]. */
int32_t tpg_maxout2_fwd(int32_t b, int32_t m, tpg_tensor x, tpg_tensor y, uint8_t* argmax, tpg_stream_t stream);
int32_t tpg_maxout2_bwd(int32_t b, int32_t m, tpg_tensor gy, const uint8_t* argmax, tpg_tensor dx,
                        tpg_stream_t stream);

/* In-place Adam (torch.optim.Adam semantics, L2 weight_decay added to the gradient) on a
 * flat fp32 buffer (the four pointers 4-byte aligned, all at the same offset inside 16 bytes).  state is a caller-owned device
 * float[4] {step, 1 - beta1^step, sqrt(1 - beta2^step), unused}, zero-initialised before the
 * first call: step > 0 sets the step count explicitly, step == 0 advances the device counter
 * by one (what a captured hipGraph replays), step < 0 leaves the counter as it is -- a slice of
 * the buffer updated under the step the last call set (the per-bucket updates of an optimizer
 * overlapped with the backward: one numel = 0, step = 0 call per step, then one step = -1 call
 * per bucket).  grad_scale multiplies the gradient. */
int32_t tpg_adam(int64_t numel, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                 float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                 float grad_scale, float* state, tpg_stream_t stream);

/* Overflow guard of the loss-scaled fp16 step (torch.cuda.amp.GradScaler's skip): state[3] :=
 * 1 if any of grad[0..numel) is inf / NaN, else 0 (device-side, graph-capturable).  A tpg_adam
 * call on the same state then leaves parameters, moments and the step counter untouched. */
int32_t tpg_grad_check(int64_t numel, const float* grad, float* state, tpg_stream_t stream);

/* ---- identity-feature extractors (MobileNetV2.py, ResNet.py, FeatureExtract.py) ---- */

/* G-step image losses (tpgan_train._g_losses, build-defined; weights config.py:59-82) fused
 * into single launches (SURVEY.md §3C loss suite).  x (the fake), r (the target), a_i, b_i:
 * logical (n, c, h, w) views of any strides, TPG_F32 / TPG_BF16 / TPG_F16; gradients are
 * written in the dtype and strides of the given tensor.  The forward writes one fp32 scalar
 * to *out (device), summing fixed per-block partials in a fixed order (deterministic); ws:
 * at least tpg_loss_workspace() bytes of device scratch.  Backward: gout = device pointer to
 * the scalar's gradient.
 *   image:  w_pix * mean|x - r| + w_sym * mean|x - flip_w(x)|
 *           + w_tv * (mean|x[y+1] - x[y]| + mean|x[:, x+1] - x[:, x]|)
 *   L1 set: sum_i weight_i * mean|a_i - b_i|   (da_i may have data NULL: no gradient) */
#define TPG_L1_MAX_SEGS 8
typedef struct tpg_l1_seg {
  int32_t n, c, h, w;
  tpg_tensor a, b, da;
  float weight;
} tpg_l1_seg;
size_t tpg_loss_workspace(void);
int32_t tpg_image_losses_fwd(int32_t n, int32_t c, int32_t h, int32_t w, tpg_tensor x, tpg_tensor r, float w_pix,
                             float w_sym, float w_tv, float* ws, size_t ws_bytes, float* out, tpg_stream_t stream);
int32_t tpg_image_losses_bwd(int32_t n, int32_t c, int32_t h, int32_t w, tpg_tensor x, tpg_tensor r, float w_pix,
                             float w_sym, float w_tv, const float* gout, tpg_tensor dx, tpg_stream_t stream);
int32_t tpg_l1_set_fwd(int32_t nseg, const tpg_l1_seg* segs, float* ws, size_t ws_bytes, float* out,
                       tpg_stream_t stream);
int32_t tpg_l1_set_bwd(int32_t nseg, const tpg_l1_seg* segs, const float* gout, tpg_stream_t stream);

/* SSD landmark head of the MobileNetV2 pretraining (MobileNetV2.py:342-649, batch 1 and per-point
 * .item() loops in the reference; here one block per image).  All pointers are fp32 / int32 / u8
 * device memory, dense:  pred (B, n, 2) pixel locations, cls (B, n, C) logits (C >= 5, class 4
 * = background), truth (B, 8) four landmarks, keys (B, n) uniform [0, 1) draws.
 *   tpg_ssd_loss_fwd  MultiTaskLoss.forward (:445-534): labels (B, n) = the landmark each anchor
 *                     is assigned to (within the k (= int(ratio * n)) nearest of a landmark, the
 *                     nearest such landmark, first on ties) or -1; sel (B, n) = 1 for the
 *                     background anchors in the class loss (all of them, or the ones with the
 *                     int(#positives * ratio_nb) smallest keys when there are more); terms
 *                     (B, TPG_SSD_TERMS): [0] alpha * loc + beta * cls, [1..4] location MSE per
 *                     landmark, [5..8] class CE per landmark, [9] background CE, [10] background
 *                     count, [11..14] positives per landmark.  n <= TPG_SSD_MAXN, 1 <= k <= n.
 *   tpg_ssd_loss_bwd  gradients of mean_b terms[b][0] times *gout (device scalar) w.r.t. pred
 *                     (dloc) and cls (dcls), from the forward's labels / sel / terms.
 *   tpg_ssd_decode    MultiTaskDecoder.forward (:551-597): per image and class, the anchors whose
 *                     softmax confidence exceeds conf, greedy NMS (suppress within nms_thr,
 *                     inclusive), the first top_k kept: keep (B, C, top_k) anchor indices (-1 =
 *                     none), score (B, C, top_k). */
#define TPG_SSD_TERMS 16
#define TPG_SSD_MAXN 4096
int32_t tpg_ssd_loss_fwd(int32_t B, int32_t n, int32_t C, const float* pred, const float* cls, const float* truth,
                         float width, float height, int32_t k, double ratio_nb, float alpha, float beta,
                         const float* keys, int32_t* labels, uint8_t* sel, float* terms, tpg_stream_t stream);
int32_t tpg_ssd_loss_bwd(int32_t B, int32_t n, int32_t C, const float* pred, const float* cls, const float* truth,
                         float width, float height, float alpha, float beta, const int32_t* labels,
                         const uint8_t* sel, const float* terms, const float* gout, float* dloc, float* dcls,
                         tpg_stream_t stream);
int32_t tpg_ssd_decode(int32_t B, int32_t n, int32_t C, const float* loc, const float* cls, float conf, float nms_thr,
                       int32_t top_k, int32_t* keep, float* score, tpg_stream_t stream);

/* Landmark front end: the detector's head outputs -> the four crop centres and crop boxes of
 * process() (DataAndDataset.py:42-54), with nothing leaving the device, and Pretrain.py's accuracy
 * measure (:17-64) for a batch.  loc / cls as above; every other pointer dense device memory unless
 * marked HOST.
 *   tpg_ssd_landmarks      per image and landmark class l in 0..3 (left eye, right eye, nose, mouth
 *                          centre) the best anchor: the largest score expf(x[l] - logsumexp(x)) --
 *                          tpg_ssd_decode's own expression, bit for bit -- the smallest index among
 *                          equal scores, a NaN score never.  This is slot 0 of tpg_ssd_decode with
 *                          top_k = 1 wherever that slot is not -1.  1 <= n <= TPG_SSD_MAXN.
 *                            scale    device float[B][2] (sx, sy) multiplied into the point in float32
 *                                     (as tpg_landmark_boxes), or NULL
 *                            patch_wh HOST int32[4][2], as tpg_landmark_boxes
 *                            points   (B, 4, 2) loc[b][anchor] (* scale); NaN when no score was a number
 *                            score    (B, 4) the best score (0 when none), anchor (B, 4) its index (-1)
 *                            boxes    (B, 4, 4) left, upper, right, lower: with x, y the floorf of the
 *                                     point, x - pw/2 + 1, y - ph/2 + 1, x + pw/2 + 1, y + ph/2 + 1
 *                            status   (B): bit l (1, 2, 4, 8) set when landmark l was not found
 *                                     (found: score > conf, strictly, as the decoder; the best
 *                                     anchor's point and box are written all the same); bit 4 (16) set
 *                                     when a chosen coordinate is NaN, infinite or |v| > 1e9 (that
 *                                     coordinate counts as 0 in the box, as tpg_landmark_boxes)
 *                          Every output slot is written on every call.
 *   tpg_landmark_accuracy  acc (B) = mean over the four landmarks of weights[i] where
 *                          thresholds[i-1] < d <= thresholds[i] (thresholds[-1] = 0), else 0, with
 *                          d = sqrtf(dx*dx + dy*dy) in float32 without FMA contraction between pred
 *                          and truth (both (B, 4, 2)).  As the reference, d == 0 scores 0; so do a NaN
 *                          d and a landmark whose bit is set in status (tpg_ssd_landmarks's; may be
 *                          NULL).  thresholds / weights: HOST float[nbands], thresholds ascending,
 *                          1 <= nbands <= TPG_LM_MAX_BANDS. */
#define TPG_LM_MAX_BANDS 8
int32_t tpg_ssd_landmarks(int32_t B, int32_t n, int32_t C, const float* loc, const float* cls, float conf,
                          const float* scale, const int32_t* patch_wh, float* points, float* score, int32_t* anchor,
                          int32_t* boxes, int32_t* status, tpg_stream_t stream);
int32_t tpg_landmark_accuracy(int32_t B, const float* pred, const float* truth, const int32_t* status, int32_t nbands,
                              const float* thresholds, const float* weights, float* acc, tpg_stream_t stream);

/* Depthwise Conv2d (groups == in_c == out_c, MobileNetV2.py:105), kernels up to 3x3, zero
 * padding: y = act(dwconv(x, w) + bias [+ res_scale * residual]).  w logical [C][1][kh][kw]
 * fp32 (any strides); x / y / residual channels-last, 16-byte aligned rows of desc.dtype. */
int32_t tpg_dwconv2d_fwd(const tpg_conv_desc* d, tpg_tensor x, tpg_tensor w, const float* bias,
                         tpg_tensor residual, tpg_tensor y, tpg_stream_t stream);
/* dx = input gradient of the depthwise conv for the masked output gradient g (overwrites dx). */
int32_t tpg_dwconv2d_bwd_data(const tpg_conv_desc* d, tpg_tensor g, tpg_tensor w, tpg_tensor dx,
                              tpg_stream_t stream);
/* dw += weight gradient (fp32 dw, logical [C][1][kh][kw]). */
int32_t tpg_dwconv2d_bwd_filter(const tpg_conv_desc* d, tpg_tensor x, tpg_tensor g, tpg_tensor dw,
                                tpg_stream_t stream);

/* MaxPool2d(k, s, p) (ResNet.py:33): padding never wins; argmax (uint8, NHWC order of y) is the
 * first window tap r*k+s attaining the maximum.  bwd overwrites dx (gather form, no atomics). */
int32_t tpg_maxpool2d_fwd(int32_t n, int32_t c, int32_t h, int32_t w, int32_t k, int32_t s, int32_t p,
                          int32_t oh, int32_t ow, tpg_tensor x, tpg_tensor y, uint8_t* argmax,
                          tpg_stream_t stream);
int32_t tpg_maxpool2d_bwd(int32_t n, int32_t c, int32_t h, int32_t w, int32_t k, int32_t s, int32_t p,
                          int32_t oh, int32_t ow, tpg_tensor gy, const uint8_t* argmax, tpg_tensor dx,
                          tpg_stream_t stream);

/* AdaptiveAvgPool2d(1) (MobileNetV2.py:173, ResNet.py:45): y[n][c] = mean over h x w
 * (y logical [n][c][1][1]); bwd: dx = gy / (h*w) broadcast (overwrites dx). */
int32_t tpg_avgpool_fwd(int32_t n, int32_t c, int32_t h, int32_t w, tpg_tensor x, tpg_tensor y,
                        tpg_stream_t stream);
int32_t tpg_avgpool_bwd(int32_t n, int32_t c, int32_t h, int32_t w, tpg_tensor gy, tpg_tensor dx,
                        tpg_stream_t stream);

/* Eval-mode BatchNorm2d folded into the preceding conv (MobileNetV2.py:100-112):
 * w_out = w * gamma / sqrt(var + eps) per output channel, b_out = (bias - mean) * that + beta
 * (bias may be NULL).  w / w_out logical [cout][cin][kh][kw] fp32, any strides. */
int32_t tpg_bn_fold(int32_t cout, int32_t cin, int32_t kh, int32_t kw, tpg_tensor w, const float* bias,
                    const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                    tpg_tensor w_out, float* b_out, tpg_stream_t stream);

/* Training-mode BatchNorm2d over N*H*W per channel (+ fused activation), pixel-dense channels-last
 * x / y of one dtype: y = act((x - mean) / sqrt(var + eps) * gamma + beta) with batch mean and
 * biased variance; save_mean / save_invstd (float[c]) are kept for the backward; running stats
 * (may both be NULL) move by momentum using the unbiased variance, as nn.BatchNorm2d.
 * ws: float[2c] scratch. */
int32_t tpg_bn_train_fwd(int32_t n, int32_t c, int32_t h, int32_t w, tpg_tensor x, const float* gamma,
                         const float* beta, float* running_mean, float* running_var, float momentum,
                         float eps, int32_t act, float slope, tpg_tensor y, float* save_mean,
                         float* save_invstd, float* ws, tpg_stream_t stream);
/* Backward of the above from dy (gradient of the activation output) and the saved y, x:
 * dx (may have data NULL) overwritten; dgamma / dbeta (may be NULL) accumulated (+=). */
int32_t tpg_bn_train_bwd(int32_t n, int32_t c, int32_t h, int32_t w, int32_t act, float slope,
                         tpg_tensor dy, tpg_tensor y, tpg_tensor x, const float* gamma,
                         const float* save_mean, const float* save_invstd, tpg_tensor dx, float* dgamma,
                         float* dbeta, float* ws, tpg_stream_t stream);

/* Data path, replaces UtilityMethods.get_5_landmarks_pixal_position
 * (UtilityMethods.py:148-164), TestDataset's landmark rescale (DataAndDataset.py:243-246) and the
 * box arithmetic of process() (DataAndDataset.py:42-54), for n faces at once.
 *   lm       device float[n][npts][2] landmark (x, y)
 *   scale    device float[n][2] (sx, sy) multiplied into the 5 points after the means, or NULL
 *   pts_idx  HOST int32[5][2] inclusive index ranges (five_pts_idx; an empty range gives NaN,
 *            as numpy's mean of an empty slice)
 *   patch_wh HOST int32[4][2] (width, height) of left_eye, right_eye, nose, mouth (40x40, 40x40, 40x32, 48x32)
 *   lm5      device float[n][5][2] the five points (before the mouth midpoint)
 *   boxes    device int32[n][4][4] (left, upper, right, lower) per patch, exactly PIL's crop box
 *   status   device int32[n]: 0, or 1 where a point was NaN/inf (the reference raises ValueError
 *            from math.floor there; the box row is then meaningless) */
int32_t tpg_landmark_boxes(int32_t n, int32_t npts, const float* lm, const float* scale, const int32_t* pts_idx,
                           const int32_t* patch_wh, float* lm5, int32_t* boxes, int32_t* status,
                           tpg_stream_t stream);
/* Crop + normalise u8 images into up to 8 outputs in one launch: out_k[b, c, y, x] =
 * u/255*2-1 with u = img[b, c, upper+y, left+x], or 0 outside the image (PIL crop fill), where
 * (left, upper) = boxes[b*box_stride + 4*slots[k] + {0, 1}], or (0, 0) when slots[k] < 0.
 *   img_stride  HOST int64[4] element strides of the u8 image's logical (n, c, h, w) view (HWC: h*w*c, 1, w*c, c)
 *   outs        HOST tpg_tensor[njobs] (f32 or bf16, logical NCHW), out_hw HOST int32[njobs][2] */
int32_t tpg_crop_normalize(int32_t n, int32_t c, int32_t in_h, int32_t in_w, const uint8_t* img,
                           const int64_t* img_stride, int32_t njobs, const tpg_tensor* outs, const int32_t* out_hw,
                           const int32_t* slots, const int32_t* boxes, int32_t box_stride, tpg_stream_t stream);
/* torchvision's ToTensor() on the device (Pretrain.py trains the landmark detector on it):
 * out[b, c, y, x] = (float)img[b, c, y, x] / 255.0f, an IEEE division, no FMA contraction, stored as
 * TPG_F32 / TPG_BF16 / TPG_F16 into a logical-NCHW tensor of any strides (channels-last in the
 * detector's compute dtype: its first conv then takes it as it is).  img_stride: HOST int64[4]
 * element strides of the u8 image's logical (n, c, h, w) view, as tpg_crop_normalize; n*h*w < 2^31. */
int32_t tpg_u8_to_unit(int32_t n, int32_t c, int32_t h, int32_t w, const uint8_t* img, const int64_t* img_stride,
                       tpg_tensor out, tpg_stream_t stream);

/* Pillow's 8-bit LANCZOS resize of RGB (HWC, 3 interleaved bands) images, byte for byte what
 * Image.resize((out_w, out_h), Image.LANCZOS) returns (DataAndDataset.py:247-251), for a batch of
 * images of DIFFERENT sizes in two launches (one per pass).  Sides are 1..4096.  Integer
 * arithmetic only on the device: per axis, out = clamp(((1 << 21) + sum_x src[xmin + x] * k[x])
 * >> 22, 0, 255) in int32, along W first into a u8 image, then along H on that rounded image; a
 * pass whose in == out is skipped.  The host side below does no device work and needs no GPU.
 *
 *   tpg_resize_ksize       taps per output sample, 2 * ceil(3 * max(in / out, 1)) + 1 (0 + message
 *                          for a size outside 1..4096)
 *   tpg_resize_coeffs      fill HOST bounds int32[out][2] = (xmin, n) and coeffs int32[out][ksize]
 *                          (weights in 22 fractional bits, zero from n on): window weights
 *                          lanczos((x + xmin - center + 0.5) * (1 / fs)) in double with libm sin,
 *                          normalised by their sum in index order, rounded half away from zero
 *   tpg_resize_table_ints  int32 count of one (in, out) table image, out * (2 + ksize): bounds then
 *                          coeffs, back to back.  The caller keeps the images of the pairs it uses
 *                          in ONE device int32 buffer and hands jobs their offsets.
 *   tpg_resize_workspace   bytes of one job's intermediate image (H x out_w x 3, rounded up to 16;
 *                          0 when either pass is skipped); negative on a bad size
 *   tpg_resize_job_bytes   size of one job record (64)
 *   tpg_resize_pack_job    write record `index` of the HOST array `jobs`; the caller uploads it.
 *                          Record layout (little endian, 64 bytes):
 *                            0 src pointer   8 row stride in bytes (>= W*3)
 *                            16 / 24 offsets (in int32) of the W-axis (W -> out_w) and H-axis
 *                                    (H -> out_h) table images in the table buffer
 *                            32 byte offset (multiple of 16) of the intermediate image in the workspace
 *                            40 H  44 W  48 out_h  52 out_w  (int32)   56 / 60 ksize of the W / H axis
 *                          Offsets of a skipped pass are ignored.  bands must be 3.
 *   tpg_resize_u8          resize njobs images into out, u8 [njobs][out_h][out_w][3].  jobs_dev,
 *                          tables_dev, out and ws are device memory; ws holds every job's
 *                          intermediate image at its offset and may be NULL when no job needs one.
 *                          A record built for another (out_h, out_w) is skipped. */
int32_t tpg_resize_ksize(int32_t in_size, int32_t out_size);
int32_t tpg_resize_coeffs(int32_t in_size, int32_t out_size, int32_t* bounds, int32_t* coeffs);
int64_t tpg_resize_table_ints(int32_t in_size, int32_t out_size);
int64_t tpg_resize_workspace(int32_t h, int32_t w, int32_t out_h, int32_t out_w);
size_t tpg_resize_job_bytes(void);
int32_t tpg_resize_pack_job(void* jobs, int32_t index, const uint8_t* src, int32_t h, int32_t w, int32_t bands,
                            int64_t row_stride, int32_t out_h, int32_t out_w, int64_t tab_h, int64_t tab_v,
                            int64_t ws_off);
int32_t tpg_resize_u8(int32_t njobs, const void* jobs_dev, const int32_t* tables_dev, int32_t out_h, int32_t out_w,
                      uint8_t* out, void* ws, tpg_stream_t stream);

/* Face alignment: the step between the landmark detector and the generator.  Fit the similarity
 * transform from a template of K points in the OUTPUT frame onto each face's K points in PHOTO
 * pixels (output frame -> photo: the direction the warp samples in, nothing is inverted), then
 * resample every photo through its matrix.  Two launches for B faces, no host round trip: the warp
 * reads the fit's 16.16 matrices from device memory.
 *
 *   tpg_similarity_fit     points: device float [B][K][2] (x, y); tmpl: HOST float [K][2], the same
 *                          for every face; 2 <= K <= 8.  Per face, in float32 with IEEE divisions,
 *                          sums over the points in index order and no FMA contraction:
 *                            qm = sum(q) / K, qc = q - qm, S = sum(qc.x*qc.x + qc.y*qc.y)  (host)
 *                            pm = sum(p) / K, pc = p - pm
 *                            a = sum(qc.x*pc.x + qc.y*pc.y) / S
 *                            b = sum(qc.x*pc.y - qc.y*pc.x) / S
 *                            tx = pm.x - (a*qm.x - b*qm.y),  ty = pm.y - (b*qm.x + a*qm.y)
 *                          matrix: float [B][6] = (a, -b, tx, b, a, ty), photo = M * out + t;
 *                          matrix_q16: int32 [B][6], each entry rint(v * 65536.0f) (ties to even);
 *                          status: int32 [B]:
 *                            bit 0 (1)  a coordinate of p is NaN, infinite or |v| > 1e9
 *                            bit 1 (2)  degenerate or out of range: a*a + b*b is zero or not finite,
 *                                       sqrt(a*a + b*b) > 32, or |tx| >= 16384 or |ty| >= 16384
 *                                       (tested only where bit 0 is clear)
 *                            bit 2 (4)  in_status[face] != 0 (in_status: device int32 [B] or NULL;
 *                                       tpg_ssd_landmarks's status, so "not found" travels on)
 *                          A face with bit 0 or bit 1 gets the identity (1, 0, 0, 0, 1, 0); every
 *                          slot of the three outputs is written on every call.  The template is
 *                          checked on the host before any device work: finite, with S > 0 and finite.
 *   tpg_warp_job_bytes     size of one job record (32)
 *   tpg_warp_pack_job      write record `index` of the HOST array `jobs`; the caller uploads it.
 *                          Record layout (little endian, 32 bytes):
 *                            0 src pointer (device, RGB u8 HWC)   8 row stride in bytes (>= W*3)
 *                            16 H  20 W  24 out_h  28 out_w  (int32)
 *                          Sides are 1..4096; bands must be 3.
 *   tpg_affine_warp_u8     out: u8 [njobs][out_h][out_w][3]; matrix_q16: device int32 [njobs][6] =
 *                          (m00, m01, tx, m10, m11, ty) in 16.16 fixed point, ANY affine map, not
 *                          only a similarity; status: device int32 [njobs].  njobs <= 65535.  Integer
 *                          arithmetic only on the device.  Per photo:
 *                            d = max(m00^2 + m10^2, m01^2 + m11^2), exact (it can reach 2^63)
 *                            n = the smallest integer in 1..16 with (n * 65536)^2 >= d; if there is
 *                                none, n = 16 and status bit 3 (8) is set: a warning, the output
 *                                is written all the same, undersampled.  Otherwise status is 0.
 *                          Per output pixel (ox, oy) and sub-sample (i, j), i, j in 0..n-1, in int64:
 *                            U = 2n*ox + 2i + 1,  V = 2n*oy + 2j + 1
 *                            X = tx + floor((m00*U + m01*V) / 2n) - 32768
 *                            Y = ty + floor((m10*U + m11*V) / 2n) - 32768
 *                          (pixel centres: output pixel ox covers [ox, ox + 1), source pixel ix has
 *                          its centre at ix + 0.5, hence the -32768).  Bilinear taps:
 *                            ix = X >> 16 (arithmetic), fx = (X >> 8) & 255; iy, fy likewise
 *                            columns ix, ix + 1 clamped to [0, W-1], rows iy, iy + 1 to [0, H-1]
 *                            weights (256 - fx, fx) x (256 - fy, fy), summing to 65536
 *                          Per channel acc = sum over sub-samples and taps of weight * pixel, and
 *                            out = (acc + 32768*n*n) / (65536*n*n)     (round half up)
 *                          So the identity matrix copies the top-left out_h x out_w of the photo
 *                          (edge-replicated beyond it), (131072, 0, 0, 0, 131072, 0) is the
 *                          round-half-up 2 x 2 box average and (0, -65536, W*65536, 65536, 0, 0) a
 *                          quarter turn.  One block per 16 x 16 output tile of one photo.  A record
 *                          built for another (out_h, out_w) is skipped: nothing of that photo is
 *                          read, and neither its slot of out nor its status word is written. */
int32_t tpg_similarity_fit(int32_t B, int32_t K, const float* points, const float* tmpl, const int32_t* in_status,
                           float* matrix, int32_t* matrix_q16, int32_t* status, tpg_stream_t stream);
size_t tpg_warp_job_bytes(void);
int32_t tpg_warp_pack_job(void* jobs, int32_t index, const uint8_t* src, int32_t h, int32_t w, int32_t bands,
                          int64_t row_stride, int32_t out_h, int32_t out_w);
int32_t tpg_affine_warp_u8(int32_t njobs, const void* jobs_dev, const int32_t* matrix_q16, int32_t out_h,
                           int32_t out_w, uint8_t* out, int32_t* status, tpg_stream_t stream);

/* Inference image path.
 *   tpg_denorm_u8  x: logical [n, c, h, w], TPG_F32 / TPG_BF16 / TPG_F16, any element strides (the
 *                  generator's outputs are channels-last views); out: u8 [n][h][w][c] contiguous
 *                  (HWC, what Image.fromarray takes), c in 1..4.  Per element in float32, no FMA
 *                  contraction: t = (float(x) + 1.0f) * 127.5f + 0.5f; out = 0 where t is NaN, else
 *                  floor(t) clamped to [0, 255] -- torchvision.utils.save_image's rounding of
 *                  (x+1)/2, and the exact inverse of tpg_crop_normalize's u/255*2-1 for all 256
 *                  byte values with x held in f32, bf16 or f16.  Loads are vector loads where x's
 *                  contiguous axis (w or c) and alignment allow; stores are dwords where out is
 *                  4-byte aligned.
 *   tpg_image_metrics_u8  a, b: u8 [n][h][w][c] contiguous, c in 1..4.  Per image:
 *                  sse[n] (int64) = sum (a - b)^2, exact;
 *                  ssim[n] (float; may be NULL, else h and w must be >= 11) = Wang et al.'s SSIM per
 *                  channel, then averaged: window g (x) g, g[k] = exp(-(k-5)^2 / (2 * 1.5^2)) / sum,
 *                  valid positions only ((h-10) x (w-10) per channel), C1 = 6.5025, C2 = 58.5225,
 *                  mu = sum w x, sigma_xy = sum w x y - mu_x mu_y (likewise sigma_x^2, sigma_y^2),
 *                  map = (2 mu_x mu_y + C1)(2 sigma_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(sigma_x^2 +
 *                  sigma_y^2 + C2)), result = mean over windows and channels.  Moments, map and
 *                  mean are float64 on the device; every sum runs in a fixed order (no atomics), so
 *                  reruns are bit-identical.
 *                  ws: device scratch, 8-byte aligned, at least tpg_image_metrics_workspace(n, h, w, c)
 *                  bytes (negative on bad sizes). */
int32_t tpg_denorm_u8(int32_t n, int32_t c, int32_t h, int32_t w, tpg_tensor x, uint8_t* out,
                      tpg_stream_t stream);
int64_t tpg_image_metrics_workspace(int32_t n, int32_t h, int32_t w, int32_t c);
int32_t tpg_image_metrics_u8(int32_t n, int32_t h, int32_t w, int32_t c, const uint8_t* a, const uint8_t* b,
                             int64_t* sse, float* ssim, void* ws, size_t ws_bytes, tpg_stream_t stream);

/* Identity scoring.  Rows are described by the first two strides of a tpg_tensor: element (r, e) of
 * a logical [n][d] view is data[r * stride[0] + e * stride[1]]; stride[2] and stride[3] are ignored.
 *   tpg_l2_normalize  x: logical [n][d], TPG_F32 / TPG_BF16 / TPG_F16, any row and element stride,
 *                  n in 0..2^24, d in 1..4096.  out: f32 [n][dpad] contiguous, dpad = d rounded up to
 *                  a multiple of 4 (anything else is rejected); columns d..dpad-1 are written as 0.
 *                  Per row: ss = sum x^2 in f32 (fmaf; lane l of a 64-lane wave adds elements l,
 *                  l + 64, ... in order, then the lanes are added by a xor butterfly: a fixed order,
 *                  reruns are bit-identical), out = x / sqrtf(ss) (correctly rounded division).
 *                  norm[n] (f32, may be NULL) = sqrtf(ss) as computed.
 *                  status[n] (int32) = 1 where an element of the row is NaN or infinite, where ss
 *                  is 0 or where ss overflowed f32; else 0.  A status-1 row is written as all zeros
 *                  (its norm is what sqrtf gave: 0, inf or NaN).
 *   tpg_cosine_topk  probes: f32 [P][dpad], gallery: f32 [G][dpad], both contiguous, 16-byte aligned,
 *                  unit rows with zero pad columns as tpg_l2_normalize writes them (the scores are
 *                  plain dot products: rows of another length give dot products, not cosines; a row
 *                  of zeros scores 0 against everything).  P and G in 0..2^24, d in 1..4096, dpad as
 *                  above, k in 1..8.
 *                  skip: int32 [P] or NULL: the gallery index probe p must not match (protocols where
 *                  the probe set is the gallery); -1, any index outside 0..G-1, or a NULL pointer
 *                  excludes nothing.
 *                  idx: int32 [P][k], score: f32 [P][k]: per probe the k best eligible gallery rows,
 *                  score descending, equal scores ordered by the lower gallery index.  Slots beyond
 *                  the number of eligible rows hold idx = -1, score = -inf.  A NaN score (a gallery or
 *                  probe row holding NaN) is never listed.
 *                  Arithmetic: v_mfma_f32_32x32x2_f32, i.e. per (probe, gallery row) one f32 fmaf
 *                  chain over the dpad columns in a fixed order that depends on neither the row's
 *                  place in a tile nor the chunking: duplicate gallery rows score bit-equal, every
 *                  gchunk gives the same scores, reruns are bit-identical.  No atomics; partial
 *                  lists are merged in chunk order.
 *                  gchunk: gallery rows per block. 0 = automatic (whole tiles of 128 rows, about
 *                  1024 blocks where the gallery allows); >= 16 forces it (tests force several chunks
 *                  at a tiny G); 1..15 is rejected.
 *                  ws: device scratch, 8-byte aligned, at least tpg_cosine_topk_workspace(P, G, k,
 *                  gchunk) bytes: one (score, index) list of k entries per probe and chunk.  The
 *                  query is positive for valid sizes (8 at least) and negative on a bad size, k or
 *                  gchunk, or where probe tiles x chunks reaches 2^31.
 *                  Two launches (search, merge); the similarity matrix is never stored.
 *   tpg_cosine_pairs  a, b: logical [n][d] as for tpg_l2_normalize, each its own dtype and strides.
 *                  cos[n] (f32) = dot / (sqrtf(|a|^2) * sqrtf(|b|^2)), the three sums in f32 in the
 *                  fixed order above.  status[n] = 1 where either row holds a NaN or infinity, has a
 *                  zero sum of squares or one that overflowed; cos is 0 there.  One launch, no
 *                  workspace.
 * Validation comes before any device work: NULL pointers (-10), sizes, k, d, dpad, gchunk (-2), dtypes
 * (-3), alignment and workspace size (-4), each with a tpg_last_error() message. */
int32_t tpg_l2_normalize(int32_t n, int32_t d, tpg_tensor x, float* out, int32_t dpad, float* norm, int32_t* status,
                         tpg_stream_t stream);
int64_t tpg_cosine_topk_workspace(int32_t P, int32_t G, int32_t k, int32_t gchunk);
int32_t tpg_cosine_topk(int32_t P, int32_t G, int32_t d, int32_t dpad, const float* probes, const float* gallery,
                        int32_t k, const int32_t* skip, int32_t gchunk, int32_t* idx, float* score, void* ws,
                        size_t ws_bytes, tpg_stream_t stream);
int32_t tpg_cosine_pairs(int32_t n, int32_t d, tpg_tensor a, tpg_tensor b, float* cos, int32_t* status,
                         tpg_stream_t stream);

/* Deterministic mode (process-wide, off by default; SURVEY.md §5 race detection): every
 * reduction runs in a fixed order — no split-K fp32 atomics in the conv forward / input
 * gradient, weight gradients with one pixel split (each dW element added once), bias
 * gradients summed by one block — so two runs on the same inputs are bit-identical.  Slower;
 * meant for parity and run-to-run tests. */
void tpg_set_deterministic(int32_t on);
int32_t tpg_get_deterministic(void);

/* Library version string and the thread-local message of the last failed call. */
const char* tpg_version(void);
const char* tpg_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TPGAN_H */
