/*
 * prpe.h — C ABI of the MI355X-native per-frame inference hot path of the
 * Person-Recognition-for-Pose-Estimation combined multi-task model.
 *
 * The reference (100 % Python, /root/reference) has no native boundary: its device work
 * is PyTorch/cuDNN operators called from nn.Modules. These entry points
 * are what a ctypes/FFI binding of that path binds; each cites the reference interface
 * (file:line) whose arithmetic it replaces. The Python host side
 * (person-recognition-for-pose-estimation_amd/prpe) mirrors the reference module API.
 *
 * Rules (all entry points):
 *   - Every buffer is caller-allocated device memory; the library never allocates.
 *   - Tensors are strided float32 views: element strides, any layout (NHWC/NCHW/...).
 *   - Calls are stream-ordered on the given hipStream_t (passed as void*), no implicit
 *     synchronisation; safe to call concurrently on different streams/devices.
 *   - Return 0 on success, a negative errno-style code (-22 = EINVAL) for bad
 *     arguments (checked before any launch), or a positive hipError_t from the launch.
 *   - Nothing throws across the ABI.
 */
#ifndef PRPE_H_
#define PRPE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRPE_ABI_VERSION 12

/* activations (epilogues/prologues) */
enum prpe_act {
  PRPE_ACT_NONE = 0,
  PRPE_ACT_RELU = 1,   /* torch.nn.ReLU */
  PRPE_ACT_SILU = 2,   /* torch.nn.SiLU  (yolopt/nets/nn.py:28-36) */
  PRPE_ACT_PRELU = 3,  /* torch.nn.PReLU, per-channel slope (libs/net_adaface.py:153-160) */
  PRPE_ACT_GELU = 4,   /* exact erf GELU (modify_models.py:356, ViT MLP) */
  PRPE_ACT_SIGMOID = 5
};

/* residual modes of the conv epilogue */
enum prpe_res_mode {
  PRPE_RES_NONE = 0,
  PRPE_RES_PRE_ACT = 1,  /* y = act(acc*scale + bias + r)   ResNet bottleneck / IR unit / ViT */
  PRPE_RES_POST_ACT = 2  /* y = act(acc*scale + bias) + r   yolopt Residual (nn.py:48-49) */
};

/* A strided 4-D float32 view, logical shape [n, h, w, c]. */
typedef struct prpe_view {
  float* ptr;
  int32_t n, h, w, c;
  int64_t sn, sh, sw, sc;
} prpe_view;

/*
 * Convolution (groups = 1) as an implicit GEMM on MFMA with split-bf16 operands
 * (fp32 accumulate): see ``precision``.
 *   y[n,oh,ow,co] = EPI( sum_{kh,kw,ci} PRO(x[n, oh*s-p+kh, ow*s-p+kw, ci]) * W[co,kh,kw,ci] )
 * PRO(v) = v*in_scale[ci] + in_bias[ci] for in-bounds taps, 0 for padding (IR-50 pre-BN,
 * libs/net_adaface.py:159). EPI = folded BN / bias (scale, bias), residual, activation.
 * Weights are packed by the host: bf16 planes [co_pad][k_pad], w = plane0 + plane1 + plane2
 * (RNE splits), with k in the order ``k_order`` names:
 *   0: k = (kh*KW+kw)*Ci + ci                          (any Ci)
 *   1: k = ((ci/32)*KH*KW + kh*KW+kw)*32 + ci%32       (Ci % 32 == 0, channel-contiguous x:
 *      the taps of one 32-channel chunk are consecutive K-steps -> input re-reads hit L1)
 * Replaces: torch.nn.Conv2d + BatchNorm2d (+act, +residual) in training/modify_models.py,
 * yolopt/nets/nn.py:28-39, libs/net_adaface.py:144-167, torchvision resnet50 (:446),
 * nn.Linear in ViTPose and IR-50 output_layer (as a 1x1 / 7x7 "conv").
 */
typedef struct prpe_conv_desc {
  prpe_view x;            /* input  [N, Hi, Wi, Ci] */
  prpe_view y;            /* output [N, Ho, Wo, Co] */
  prpe_view res;          /* residual [N, Ho, Wo, Co] (ptr may be NULL) */
  int32_t kh, kw, stride, pad;
  const uint16_t* w_hi;   /* bf16 bits, plane 0 */
  const uint16_t* w_lo;   /* plane 1 (precision 0, 2) */
  const uint16_t* w_lo2;  /* plane 2 (precision 2) */
  int32_t k_pad, co_pad;  /* packed extents (k_pad % 32 == 0, co_pad % 128 == 0) */
  const float* scale;     /* [Co] or NULL (= 1) */
  const float* bias;      /* [Co] or NULL (= 0) */
  const float* slope;     /* [Co] PReLU slopes or NULL */
  const float* in_scale;  /* [Ci] or NULL; needs the vector path (x.sc == 1, Ci % 4 == 0, 16-B rows) */
  const float* in_bias;   /* [Ci] or NULL */
  int32_t act;            /* prpe_act */
  int32_t res_mode;       /* prpe_res_mode */
  int32_t precision;      /* 0 = 2-plane split-bf16, 3 MFMA terms (~2^-17);
                             2 = 3-plane split (exact fp32 operands), 6 terms;
                             3 = 2-plane split-fp16 with power-of-2 scaling, 3 terms (~2^-21
                                 per operand: below fp32 accumulation error for K >= 64);
                                 needs w_h16/w_l16/scale16/x_amax, no in_scale, and a
                                 channel-chunked input (Ci % 32 == 0, k_order 1 or 1x1);
                             4 = ONE fp16 plane per operand with the same power-of-2 scaling,
                                 RNE, 1 term (~2^-12 per operand); needs w_h16/scale16/x_amax
                                 (w_l16 unused), a channel-chunked input, no dual input / planes;
                                 in_scale allowed (the kernel bounds max|PRO(x)| by
                                 x_amax max|in_scale| + max|in_bias|); the AdaFace branch's policy;
                             1 = plain bf16 (1 term; diagnostics only) */
  int32_t tile;           /* 0 = auto; 1..6 = 128x128, 128x64, 128x32, 128x16, 256x128, 256x64
                             (register-staged); 10..12 LDS-DMA staged; 21..25 wave-row */
  int32_t k_order;        /* weight K order, see above */
  /* precision 3 operands: fp16 planes [co_pad][k_pad] of w[co][k] * 2^e[co] (w = (h16 + l16)
   * * 2^-e[co] to ~2^-22), the epilogue scale with 2^-e[co] folded in, and PER-FRAME bounds
   * x_amax[n] >= max|x[n]| (n < N; the producer's y_amax) that set each frame's power-of-2
   * activation scale -- a frame's arithmetic never depends on the other frames of the batch */
  const uint16_t* w_h16;
  const uint16_t* w_l16;
  const float* scale16;   /* [Co] */
  const float* x_amax;    /* [N] device */
  float* y_amax;          /* optional (any precision): device [N], y_amax[n] raised to max|y[n]|
                             (atomic; zero it before the producing launch) */
  /* optional second input (x2.ptr != NULL): y = EPI(W[:, :Ci] x + W[:, Ci:] x2), a 1x1 unpadded
   * conv over both; x2 is [N, Ho, Wo, C2] on the output's pixel grid (any strides, e.g. a
   * stride-2 subsampling view), channel-contiguous, C2 % 32 == 0 and Ci % 32 == 0; weights
   * packed [co_pad][k_pad] with k = Ci + C2 columns; precision 0/2/3 (3 also needs x2_amax [N];
   * one activation scale per frame for both inputs). Replaces a ResNet bottleneck's conv3 + downsample
   * projection + residual add (torchvision resnet50 Bottleneck.forward) with one GEMM. */
  prpe_view x2;
  const float* x2_amax;
  /* planes format: a tensor of fp32 shape [N,H,W,C] whose bytes hold, per pixel and per
   * group of 8 channels, the 8 bf16 hi planes then the 8 bf16 lo planes of the two-plane split
   * (hi = RNE(v), lo = RNE(v - hi)): what precision 0 would compute from the fp32 values, so a
   * producer that writes it saves the consumer's split, bit for bit. x_planes: x is in it
   * (precision 0, channel-chunked 1x1/3x3, wave-row kernel); y_planes: write y in it
   * (channel-contiguous, C % 8 == 0, 32-B aligned). */
  int32_t x_planes;
  int32_t y_planes;
  /* optional 1x1 GEMM in the epilogue (w2 != NULL): after scale/bias/act, z = y' W2^T with W2
   * fp32 [y2.c][Co], written to y2 [N, Ho, Wo, y2.c] (channel-contiguous, y2.c <= 32) instead
   * of y (not written). Split-bf16 matrix-core products (two planes per operand, three
   * products: the precision-0 split) on the tile held in LDS. The 3x3 conv -> Co <= 4 3x3 conv
   * pairs of the adapters (the second conv as its 1x1 tap GEMM + shifted tap sum,
   * prpe_upconv3x3 at unit scale): the intermediate tensor never reaches HBM. Haloed-tile 3x3
   * kernel only (3x3 / s1 / p1, Co <= 128, precision 0 or 3, no residual / planes / max|y|). */
  const float* w2;
  prpe_view y2;
  /* optional second stage (w3 != NULL, with w2): z1 = act2(scale2 * (y' W2^T) + bias2) with
   * W2 fp32 [n2][Co], n2 <= 64 (scale2 / bias2 [n2] or NULL for 1 / 0), then z = z1 W3^T with
   * W3 fp32 [y2.c][n2] into y2 (a conv -> 1x1 conv -> tap GEMM chain, YOLO adapter .10/.13/.16) */
  const float* w3;
  const float* scale2;
  const float* bias2;
  int32_t act2;
  int32_t n2;
  /* caller-owned device scratch, >= prpe_conv2d_workspace_bytes(d) bytes, 256-B aligned (NULL and
   * 0 when that is 0). Only the split-K path of full-window linears uses it (the IR-50 output
   * layer: partial sums per K-slice); a call that needs more than it is given returns -EINVAL.
   * Concurrent calls on different streams must pass different workspaces. */
  void* workspace;
  int64_t workspace_bytes;
} prpe_conv_desc;

/* Scratch bytes prpe_conv2d(d) needs (0 for every path but split-K), or -EINVAL for a descriptor
 * prpe_conv2d would reject. Host-only: no launch, no allocation. */
int64_t prpe_conv2d_workspace_bytes(const prpe_conv_desc* d);
int prpe_conv2d(const prpe_conv_desc* d, void* stream);

/*
 * Fused ResNet bottleneck with identity shortcut, precision 3 (torchvision Bottleneck.forward,
 * v1.5; the reference trunk's layer1 blocks 1-2, modify_models.py:413-446):
 *   y = relu(bn3(conv3(relu(bn2(conv2_3x3(relu(bn1(conv1(x)))))))) + x)
 * x, y: [N, H, W, 4*mid] channel-contiguous (x 16-B aligned rows; x [N, H, W, mid] for the
 * projection block below); x_amax [N] per-frame max|x|
 * (as prpe_conv2d precision 3); y_amax (optional) raised to max|y[n]|. Weights as prpe_conv2d's
 * precision-3 packs: fp16 planes w_h16 / w_l16 [co_pad][k_pad] (conv1 k = 4 mid, conv2 chunk-major
 * k = 9 mid, conv3 k = mid), scale16 (the planes' 2^-e folded in) and bias [Co]. The two inner
 * activations never reach HBM; they are rounded to fp16 planes with one power-of-2 scale per
 * 8 x 16 output tile (per frame and tile: frames stay independent). mid = 64 (layer1) or 128
 * (layer2, identity blocks only).
 * Projection block (layer1.0, stride 1): x has mid channels (x.c == mid, y.c == 4 mid) and
 *   y = relu(bn3(conv3(t2)) + bn_d(downsample(x)))
 * with conv3 and the downsample 1x1 as ONE dual GEMM over [t2 | x]: weight slot 2 is then the
 * [4 mid][2 mid] matrix [s3 W3 | sd Wd] (both BN scales folded into its rows, k_pad = 2 mid) and
 * bias[2] = b3 + bd; t2 and x share one power-of-2 scale (max of the tile's max|t2| and the
 * frame's max|x|), as prpe_conv2d's dual-input GEMM.
 * x, y, the weight planes, scale16 and bias 16-B aligned, x / y pixel strides multiples of 4
 * floats, one frame of x and of y < 2^31 bytes; anything else returns -EINVAL. Not in place: y
 * must not overlap x (other tiles read x's halo and residual while y is written) -> -EINVAL.
 */
typedef struct prpe_bneck_desc {
  prpe_view x;
  prpe_view y;
  const float* x_amax;
  float* y_amax;
  int32_t mid;
  const uint16_t* w_h16[3];
  const uint16_t* w_l16[3];
  int32_t k_pad[3];
  const float* scale16[3];
  const float* bias[3];
} prpe_bneck_desc;
int prpe_bottleneck(const prpe_bneck_desc* d, void* stream);

/*
 * ResNet-50 stem + max-pool in one launch, precision 3 (torchvision resnet50 conv1 7x7/2 pad 3
 * -> bn1 -> relu -> maxpool 3x3/2 pad 1; the reference trunk, modify_models.py:413-446):
 *   y[n, py, px, c] = max over the 3x3 / 2 window of relu(bn1(conv1(x)))
 * x: the frames as a zero-bordered NHWC4 buffer, element (n, h, w, c) at x + n*xsn + h*xsh + 4*w + c,
 * h < H + 6, w < W + 8, the image at rows / columns 3 .. (prpe_copy_pad writes it; the 4th
 * channel and the border are zero); x_amax [N] per-frame max|x|. The weight pack is the stem's
 * precision-3 pack of prpe_conv2d's chunked form: W'[64][224], k = kh*32 + kw*4 + c (zero for
 * kw = 7, c = 3), fp16 planes w_h16 / w_l16 with scale16 (2^-e folded in) and bias [64]. Every
 * stem value equals prpe_conv2d's on the same view bit for bit; the stem map never reaches HBM.
 * y: [N, H/4, W/4, 64], channel-contiguous, 16-B aligned; y_amax (optional) raised to max|y[n]|
 * (= the stem map's max: every stem output lies in some window). H, W multiples of 4, one frame
 * of x < 2^31 bytes, y not overlapping x's N frames; anything else returns -EINVAL.
 */
typedef struct prpe_stem_desc {
  const float* x;
  int64_t xsn, xsh;
  int32_t n, h, w;
  const float* x_amax;
  const uint16_t* w_h16;
  const uint16_t* w_l16;
  int32_t k_pad;
  const float* scale16;
  const float* bias;
  prpe_view y;
  float* y_amax;
} prpe_stem_desc;
int prpe_stem_maxpool(const prpe_stem_desc* d, void* stream);

/*
 * conv3x3(pad 1) o bilinear-upsample, second stage of the exact algebraic rewrite
 *   conv3x3(U(x)) = sum_tap shift_tap(U(Z_tap)),   Z_tap = W_tap . x  (low-res 1x1 GEMM)
 * z: [N, Hi, Wi, 9*Co] low-res per-tap products (channel = tap*Co + co, tap = kh*3+kw).
 * y[n,oy,ox,co] = act( (sum_tap valid * bilerp(Z_tap, src(oy+kh-1, ox+kw-1))) * scale + bias )
 * align_corners = 1: src = dst*(in-1)/(out-1);  0: src = max(0,(dst+0.5)*in/out-0.5).
 * Replaces nn.Upsample(bilinear) + Conv2d(3x3) + BN + act in modify_models.py:47-52,
 * :237-242, :359-364 and the ViTPose simple decoder (modeling_vitpose.py:120-144).
 * workspace = NULL (the product path) selects the fused one-pass kernel: x-interpolated
 * source rows are kept in rolling registers, HBM traffic = y write + z read. With a workspace
 * of >= prpe_upconv3x3_workspace_bytes(z, y) bytes the sum is instead evaluated in two passes
 * through it (x-interpolation, then y; kept for ablation). Both agree to fp32 rounding.
 * y_planes: write y in the planes format described at prpe_conv_desc: fused path, C % 8 == 0,
 * channel-contiguous, 32-B aligned; for a precision-0 consumer conv.
 * y_amax (optional, ABI 8): device [N], y_amax[n] raised to max|y[n]| (zeroed by the caller;
 * the per-frame bound a precision-3/4 consumer conv reads as its x_amax); fused path only.
 */
int64_t prpe_upconv3x3_workspace_bytes(const prpe_view* z, const prpe_view* y);
int prpe_upconv3x3(const prpe_view* z, const prpe_view* y, int32_t align_corners,
                   const float* scale, const float* bias, const float* slope, int32_t act,
                   int32_t y_planes, float* y_amax, void* workspace, int64_t workspace_bytes,
                   void* stream);

/* Depthwise kxk conv (groups = C) + folded BN + act (+ post-act residual add when res.ptr).
 * Replaces yolopt Conv(g=ch) (nn.py:108, :248-250). */
int prpe_dwconv(const prpe_view* x, const prpe_view* y, const prpe_view* res,
                const float* w /* [C][k][k] */, int32_t k, int32_t stride, int32_t pad,
                const float* scale, const float* bias, int32_t act, void* stream);

/* Max pooling, k x k / stride / pad (-inf padding). torchvision resnet maxpool,
 * yolopt SPP (nn.py:88-94), IR-50 MaxPool2d(1, s) shortcut (net_adaface.py:148). */
int prpe_maxpool(const prpe_view* x, const prpe_view* y, int32_t k, int32_t stride,
                 int32_t pad, void* stream);

/* Strided copy with channel zero-padding: y[...,c] = c < x.c ? x[...,c] : 0 (e.g. NCHW frames
 * -> NHWC4 for the vectorised stem conv; the 4th channel meets a zero weight column).
 * y_amax (optional): device [N], y_amax[n] raised to max|y[n]| (zeroed by the caller). */
int prpe_copy_pad(const prpe_view* x, const prpe_view* y, float* y_amax /* optional */, void* stream);

/* Nearest x2 upsample (yolopt DarkFPN nn.Upsample(scale_factor=2), nn.py:195). */
int prpe_upsample_nearest2x(const prpe_view* x, const prpe_view* y, void* stream);

/* Per-sample, per-channel standardisation + sigmoid (modify_models.py:84-86):
 * y = sigmoid((x - mean_hw) / (std_hw_unbiased + 1e-6)). */
int prpe_norm_sigmoid(const prpe_view* x, const prpe_view* y, void* stream);

/* LayerNorm over the last dim of rows (ViTPose, eps 1e-12). x/y: [rows][C] with row strides.
 * flags: bit 0 = ReLU on the output (simple decoder's ReLU, modeling_vitpose.py:139); bit 1 =
 * write y in the planes format described at prpe_conv_desc: C % 8 == 0, C <= 1024, 16-B aligned x rows,
 * 32-B aligned y rows; the input format of the precision-0 GEMM that consumes it. */
int prpe_layernorm(const float* x, int64_t x_row_stride, float* y, int64_t y_row_stride,
                   int64_t rows, int32_t C, const float* gamma, const float* beta,
                   float eps, int32_t flags, void* stream);

/* ViT multi-head self-attention, softmax(Q K^T * scale) V per (frame, head).
 * qkv: [B*L][3*H*D] rows (q | k | v, head-major inside each), out: [B*L][H*D].
 * Replaces eager_attention_forward (modeling_vitpose_backbone.py:100-126). */
int prpe_attention(const float* qkv, float* out, int32_t B, int32_t L, int32_t H, int32_t D,
                   float scale, void* stream);

/* The same attention on a strided q/k/v operand: element (frame b, which w = 0 q / 1 k / 2 v,
 * head h, token t, channel d) at qkv[b*s_frame + w*s_which + h*s_head + t*s_tok + d]; all
 * strides multiples of 4 elements, qkv 16-B aligned. prpe_attention is the row-major case
 * (s_frame = L*3*H*D, s_which = H*D, s_head = D, s_tok = 3*H*D); a head-major QKV GEMM output
 * [B][3][H][L][D] (s_frame = 3*H*L*D, s_which = H*L*D, s_head = L*D, s_tok = D) gives every
 * head's K and V as one contiguous 48-KB block. out: [B*L][H*D], in the planes format of
 * prpe_conv_desc when out_planes != 0 (the input format of the precision-0 projection GEMM). */
int prpe_attention_strided(const float* qkv, int64_t s_frame, int64_t s_which, int64_t s_head,
                           int64_t s_tok, float* out, int32_t B, int32_t L, int32_t H, int32_t D,
                           float scale, int32_t out_planes, void* stream);

/* YOLO PSA attention core (nn.py:111-122): per frame, per head:
 *   out[c, i] = sum_j v[c, j] softmax_j(q[:, i] . k[:, j] * scale)
 * qkv view [N, h, w, nh*(2*dk+dh)] (per head: q dk | k dk | v dh), out view [N,h,w,nh*dh].
 * vout (optional, ptr may be NULL): v gathered head-major [N,h,w,nh*dh] — the
 * ``v.reshape(b, c, h, w)`` operand of the depthwise positional conv (nn.py:122).
 * out (and vout) must have qkv's N, h and w: any other map size is PRPE_EINVAL. */
int prpe_psa_attention(const prpe_view* qkv, const prpe_view* out, const prpe_view* vout,
                       int32_t nh, int32_t dk, int32_t dh, float scale, void* stream);

/* YOLO Head eval decode (nn.py:255-270 + DFL nn.py:212-225 + make_anchors util.py:85-96).
 * head: [B, A, 64+nc] rows (per anchor: 64 DFL logits, nc class logits), levels given by
 * (h_l, w_l, stride_l) in anchor order; out: [B, 4+nc, A] = (cx,cy,w,h)*stride, sigmoid(cls). */
int prpe_dfl_decode(const float* head, float* out, int32_t B, int32_t nc, int32_t nlevels,
                    const int32_t* level_hw /* [nlevels*2] host */, const float* strides /* host */,
                    void* stream);

/* Row-wise L2 normalisation: norm = ||x||_2, emb = x / max(norm, eps).
 * eps = 0: IR-50 output torch.div(x, norm) (net_adaface.py:334-337; a zero row gives NaN as there);
 * eps = 1e-12: F.normalize (face_recognition/module.py:137-138; a zero row gives 0). */
int prpe_l2norm(const float* x, float* emb, float* norm, int32_t rows, int32_t C, float eps, void* stream);

/*
 * yolopt.util.non_max_suppression (training/yolopt/util.py:123-169), batched, on device.
 * pred: [B, 4+nc, N] when layout = 0; [B, N, 4+nc] when layout = 1 (same arithmetic as the
 * reference on a transposed tensor). Candidates: max class score > conf; boxes cxcywh ->
 * xyxy; nc==1: best class; nc>1: every (box, class) with score > conf; stable descending
 * score order (ties by index), <= max_nms candidates, class offset 7680*cls,
 * greedy suppression IoU > iou (torchvision.ops.nms), <= max_det kept.
 * out: [B, max_det, 6] (x1,y1,x2,y2,conf,cls), count: [B] int32. No host sync.
 * workspace: >= prpe_nms_workspace_bytes(B, N, nc, max_nms) bytes, 256-B aligned (0 bytes and
 * NULL allowed when N*nc <= 16384: candidates sorted in LDS; above that the keys and one
 * rocPRIM radix sort per image go through the workspace).
 * The reference's wall-clock cut-off (util.py:133-134,166-167) is not reproduced.
 */
int64_t prpe_nms_workspace_bytes(int32_t B, int32_t N, int32_t nc, int32_t max_nms);
int prpe_nms(const float* pred, int32_t B, int32_t N, int32_t nc, int32_t layout,
             float conf, float iou, int32_t max_nms, int32_t max_det,
             float* out, int32_t* count, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * PoseEstimationModule._get_keypoints_from_heatmaps (pose_estimation/module.py:237-296):
 * per (frame, keypoint) softmax over H*W, coords = (E[x]+0.5)/W, (E[y]+0.5)/H, score =
 * max prob (* clamp(sqrt(box area)/96, .5, 2) when boxes != NULL, boxes [B,4] x1y1x2y2).
 * heat: [B, K, H, W] contiguous. argmax (optional, may be NULL): [B,K] int32 flat index of
 * the max (first occurrence) = the hard-argmax keypoint.
 */
int prpe_softargmax(const float* heat, int32_t B, int32_t K, int32_t H, int32_t W,
                    const float* boxes, float* coords, float* scores, int32_t* argmax,
                    void* stream);

/*
 * Pose flip test, device half (pose_estimation/module.py:470-484):
 *   out = (heat + F) * 0.5,  F[b,k,h,w] = heat_flipped[b', k', h, W-1-w]
 * heat_flipped = heatmaps of the W-flipped frames. partner[k] (host, K <= 64) = the other
 * keypoint of k's flip pair or -1. mode 0 = the reference's arithmetic: for paired channels
 * ``flipped[:, pair].flip(0)`` reverses the BATCH order (b' = B-1-b, k' = k); mode 1 = the
 * channel swap the code intends (b' = b, k' = partner[k]). out must not alias heat_flipped.
 */
int prpe_flip_average(const float* heat, const float* heat_flipped, float* out, int32_t B, int32_t K,
                      int32_t H, int32_t W, const int32_t* partner, int32_t mode, void* stream);

/*
 * Face-recognition eval head, row reductions (face_recognition/module.py:141-145):
 * logits [B, C] (row stride ld) = s * cos(normalize(emb), normalize(kernel)) from prpe_conv2d.
 * argmax[b] = first index of the row max (torch.max(1)[1]); with labels (int64 [B]):
 * loss[b] = logsumexp(row) - row[label]; summary (optional, [2]) = mean loss
 * (F.cross_entropy) and mean(argmax == label) (the reference's acc).
 */
int prpe_ce_argmax(const float* logits, int64_t ld, int32_t B, int32_t C, const int64_t* labels,
                   float* loss, int32_t* argmax, float* summary, void* stream);

/*
 * Detection eval metrics (DetectionMetrics, training/lightning/face_detection/module_v2.py:13-127,
 * as driven by validation_step :458-499). State is caller-allocated on
 * the device: counters uint64 [4] = (tp, fp, gt, records), zeroed to reset; records float
 * [capacity][2] = (score, best IoU) appended in image, then prediction order.
 * update: dets [B, max_det, 6] (x1,y1,x2,y2,conf,cls) + counts [B] from prpe_nms, ground truth
 * gt_boxes [G, 4] xyxy with gt_batch [G] (int64 image index, the reference's targets['batch_idx']);
 * images with no prediction or no ground truth are skipped (validation_step's `continue`s);
 * each prediction's best IoU over its image's boxes (box_iou: inter / (union + 1e-6), fp32),
 * tp if > 0.5. Records past capacity are dropped (counters[3] still counts them).
 * compute (epoch end): n = counters[3] (host value), thresholds = host float[10]
 * (torch.linspace(0.5, 0.95, 10)); out double[6] = precision, recall, f1, mAP50, mAP75, mAP
 * (compute(): stable descending sort by score, per-threshold cumulative tp/fp, torch.trapz).
 */
int64_t prpe_det_metrics_update_workspace_bytes(int32_t B);
int prpe_det_metrics_update(const float* dets, const int32_t* counts, int32_t B, int32_t max_det,
                            const float* gt_boxes, const int64_t* gt_batch, int32_t G, uint64_t* counters,
                            float* records, int64_t capacity, void* workspace, int64_t workspace_bytes,
                            void* stream);
int64_t prpe_det_metrics_compute_workspace_bytes(int64_t n);
int prpe_det_metrics_compute(const uint64_t* counters, const float* records, int64_t n,
                             const float* thresholds, double* out, void* workspace, int64_t workspace_bytes,
                             void* stream);

/*
 * Detection eval loss (FaceDetectionModule.compute_loss, module_v2.py:178-303, as validation_step
 * :467 calls it on the eval head output): boxes [B, 4, N] and scores [B, C, N] as strided views
 * (element strides [3] each, host arrays), ground truth gt_boxes [G, 4] / gt_batch [G] / optional
 * gt_classes [G] (int64). per_image [B][4] = (loss_b, box, cls, bg) (NaN where the reference
 * computes no such term), loss [1] = sum_b loss_b / B. N <= 1024. See csrc/detmetrics.hip.
 */
int prpe_det_eval_loss(const float* boxes, const int64_t* box_strides, const float* scores,
                       const int64_t* score_strides, int32_t B, int32_t C, int32_t N, const float* gt_boxes,
                       const int64_t* gt_batch, const int64_t* gt_classes, int32_t G, float* per_image,
                       float* loss, void* stream);

/*
 * Pose validation step after the model (PoseEstimationModule.validation_step,
 * pose_estimation/module.py:486-502), one 256-thread workgroup per (frame, keypoint), no target
 * tensor in memory. pred = heat, or (heat + F) * 0.5 with prpe_flip_average's F / partner / mode
 * when heat_flipped != NULL (avg_out, optional, then receives pred; it must not overlap
 * heat_flipped, it may be heat itself (in place) but must not overlap heat otherwise, and
 * without heat_flipped it must be NULL).
 *   target (_generate_target_heatmap :298-380): keypoints [B,N,K,3] = (x, y normalised, v),
 *     mu = (x*W - 0.5, y*H - 0.5), sigma_n = sigma * clamp(sqrt(areas[b,n])/96, .5, 2) (areas
 *     [B,N]; NULL: sigma), max over instances of exp(-(dx^2+dy^2) / (2 sigma_n^2)) * (v > 0),
 *     / (sum_hw + 1e-8), zeroed where <= 0.005. An instance whose K visibilities are all 0 is
 *     skipped (:348-350); weight = max over the other instances of (v == 2 ? 1 : 0.5), so an
 *     invisible keypoint of a processed instance weighs 0.5 (:369-372).
 *   loss (JointsMSELoss :60-111): per_kp [B,K] = mean_hw((pred - target)^2) * weight *
 *     kp_weights[k] (host float[K]); a second launch writes loss[1] = sum_b (sum of the topk
 *     largest per_kp[b,:]) / (B*topk) in a fixed order (no atomics: the same bits every run).
 *   soft-argmax (_get_keypoints_from_heatmaps :237-296) of pred: coords [B,K,2], scores [B,K],
 *     argmax (optional) exactly as prpe_softargmax gives them on pred; boxes [B,N,4] (optional):
 *     instance 0's box scales the scores (boxes[:, 0], :501).
 * target_out [B,K,H,W] / weights_out [B,K] (optional) receive the target and its weights.
 * K <= 64, 1 <= N <= 256, 1 <= topk <= K; any H, W. -EINVAL launches nothing.
 */
int prpe_pose_eval_loss(const float* heat, const float* heat_flipped, const int32_t* partner, int32_t mode,
                        float* avg_out, int32_t B, int32_t K, int32_t H, int32_t W, const float* keypoints,
                        const float* areas, const float* boxes, int32_t N, float sigma, const float* kp_weights,
                        int32_t topk, float* per_kp, float* loss, float* coords, float* scores, int32_t* argmax,
                        float* target_out, float* weights_out, void* stream);

/*
 * COCO keypoint records of the pose validation step (pose_estimation/module.py:505-561) without
 * host syncs. coords [B,K,2] / scores [B,K] from prpe_pose_eval_loss; boxes [B,N,4] xyxy, areas
 * [B,N], masks / is_crowd [B,N] uint8; keep [B] uint8, a HOST array (it travels in the kernel
 * arguments: no upload, no synchronisation) = 1 where the host has not seen the image id before
 * in this epoch (:510-513). For a kept image b and n in range(sum(masks[b]))
 * (the COUNT of true masks, as :516 iterates), crowd instances skipped (:517), one record:
 *   rec_kpts [capacity,K,3] = (kx*(x2-x1) + x1, ky*(y2-y1) + y1, score > keypoint_thresh ? 2 : 1)
 *     (fp32 multiply, then fp32 add; the comparison in double as .item() > thresh does),
 *   rec_meta [capacity,8]  = (slot_base + b, n as int32 bits; mean of the K scores, box x 4, area).
 * State is caller-allocated on the device as for prpe_det_metrics_update: counter uint64 [1],
 * zeroed to reset. Records are appended in (image, instance) order at *counter; records past
 * capacity are dropped while the counter keeps counting. K <= 64.
 */
int prpe_pose_coco_records(const float* coords, const float* scores, const float* boxes, const float* areas,
                           const uint8_t* masks, const uint8_t* is_crowd, const uint8_t* keep, int32_t B,
                           int32_t N, int32_t K, double keypoint_thresh, int32_t slot_base, uint64_t* counter,
                           float* rec_kpts, float* rec_meta, int64_t capacity, void* stream);

/*
 * Top-down pose: person boxes -> ViTPose crops -> keypoints in frame pixels, all on the device
 * (csrc/topdown.hip). The reference has no runnable crop stage
 * (pose_estimation/datamodule_v2.py leans on packages that are not part of it), so the semantics
 * are defined here; the resample equals torch's grid_sample(bilinear, zeros, align_corners=False).
 *
 * crop_meta [max_crops][8] float: frame index and detection row as int32 bits (as rec_meta), the
 * window x0, y0, w, h in frame pixels, the detection score, one spare column (0).
 *
 * select: dets [B, max_det, 6] + counts [B] from the padded NMS (rows in descending score order).
 *   A frame's candidates are its first rows with score >= score_thr, at most max_per_frame of them;
 *   of these a row is skipped when a scaled coordinate (x * box_scale_x, y * box_scale_y) or its
 *   window is not finite or a scaled side is below min_size. counts[b] < 0 (NMS candidate
 *   overflow): nothing from b, status bit 0. Slots go in (frame, row) order by a scan inside one
 *   workgroup: the same list every run. Crops past max_crops are dropped from the end, status bit
 *   1. n_crops [1] = slots filled; slots at or past it get frame index -1 (other columns 0).
 *   Window, fp32, in this order (a = 192/256): cx = (x1+x2)*0.5, cy = (y1+y2)*0.5; w = x2-x1,
 *   h = y2-y1; w > a*h ? h = w/a : w = h*a; w *= pad, h *= pad; x0 = cx - 0.5*w, y0 = cy - 0.5*h.
 *   H, W (the frame, 1..2^24) are validated only: a window is not clipped to the frame.
 * resize: frames = a strided view [B, H, W, 3] (any strides, e.g. NCHW frames permuted);
 *   crops = the contiguous, 16-byte aligned, zero-bordered NHWC4 buffer [max_crops, 260, 196, 4].
 *   Slot s < *n_crops: crops[s, 2+i, 2+j, 0:3] = bilinear sample at
 *   (x0 + (j+0.5)*w/192 - 0.5, y0 + (i+0.5)*h/256 - 0.5), taps outside the frame 0. Slots at or
 *   past *n_crops (and slots whose frame index is outside [0, B)): interior zeros. The border is
 *   never written; channel 3 only ever receives 0. n_crops and crop_meta are read on the device.
 * keypoints: coords [n, K, 2] in [0,1] of the crop + scores [n, K] (prpe_softargmax on the crops'
 *   heatmaps), n <= max_crops the slots the pose net ran on. kpts [max_crops, K, 3] =
 *   (x0 + cx*w, y0 + cy*h, score) (fp32 product, then sum) for slots below min(*n_crops, n),
 *   zeros above.
 * -EINVAL launches nothing.
 */
int prpe_crop_select(const float* dets, const int32_t* counts, int32_t B, int32_t max_det, float score_thr,
                     int32_t max_per_frame, float min_size, float box_scale_x, float box_scale_y, int32_t H,
                     int32_t W, float pad, int32_t max_crops, float* crop_meta, int32_t* n_crops, int32_t* status,
                     void* stream);
int prpe_crop_resize(const prpe_view* frames, const float* crop_meta, const int32_t* n_crops, int32_t max_crops,
                     float* crops, void* stream);
int prpe_crop_keypoints(const float* coords, const float* scores, int32_t n, int32_t K, const float* crop_meta,
                        const int32_t* n_crops, int32_t max_crops, float* kpts, void* stream);

/*
 * uint8 frames in (csrc/ingest.hip): what a camera, a decoder or a dataloader hands
 * over -- uint8 HWC images at the source resolution, RGB or BGR -- resized, normalised and written
 * straight into the buffer the next kernel reads. The reference resizes with cv2 (A.Resize +
 * A.Normalize, object_detection/datamodule.py:78-100, pose_estimation/datamodule.py:374-395), whose
 * uint8 fixed-point rounding is not restated here; the semantics are this project's: half-pixel-
 * centre bilinear, no antialias, per-channel affine, all in fp32 on the raw 0..255 values.
 *
 * A strided 4-D uint8 view, logical shape [n, h, w, c], strides in elements (= bytes): an HWC
 * batch, NCHW frames through a permute, a slice of a wider tensor.
 */
typedef struct prpe_view_u8 {
  const uint8_t* ptr;
  int32_t n, h, w, c;
  int64_t sn, sh, sw, sc;
} prpe_view_u8;

/*
 * frame_ingest: frames [B, Hs, Ws, 3] uint8 -> y, the interior [B, H, W, 4] of the stem's
 * zero-bordered NHWC4 buffer (4 contiguous channels, 16-byte aligned, strides multiples of 4
 * floats: what the 16-byte path of the strided copy asks of its destination). The geometry comes
 * from the host: the region (top, left, nh, nw) inside H x W; stretch is (0, 0, H, W), a letterbox
 * a centred region (prpe/ingest.py).
 *   Inside the region, pixel (i, j) samples the source at
 *     sx = clamp((j - left + 0.5) * (Ws / nw) - 0.5, 0, Ws - 1),
 *     sy = clamp((i - top  + 0.5) * (Hs / nh) - 0.5, 0, Hs - 1)      (edges replicate: torch's
 *   F.interpolate(bilinear, align_corners=False, antialias=False)). Coordinates in fp64, each
 *   weight ax = sx - floor(sx), ay rounded to fp32 once; on the raw values, fp32:
 *     t = v00 + ax * (v01 - v00), u = v10 + ax * (v11 - v10), raw = t + ay * (u - t).
 *   y[.., c] = raw * a[c] + b[c], an fp32 multiply, then an fp32 add (never fused): at nh == Hs and
 *   nw == Ws the output has the bits of torch's u8.float() * a + b. swap_rb != 0: output channel c
 *   reads source channel 2 - c (BGR sources); a, b, fill are indexed by the OUTPUT channel.
 *   Outside the region: y[.., c] = fill[c] * a[c] + b[c] (fill in raw units). Channel 3 = 0, in the
 *   same 16-byte store. The buffer's border is never addressed.
 * a, b, fill: HOST arrays of 3 floats; they travel in the kernel arguments (no upload).
 * y_amax (optional): device [B], y_amax[n] raised to max|y[n]| over the whole interior, fill
 *   pixels included (zeroed by the caller).
 * -EINVAL, nothing launched: a null pointer, frames->c != 3, frames->n != y->n, a source or
 *   destination side below 1 (or a source side above 2^24), y not 4 contiguous 16-byte aligned
 *   channels, a region that is empty or not inside H x W, a grid past 31 bits. No argument makes
 *   the kernel read outside the source: coordinates are clamped before they become indices.
 *
 * crop_resize_u8: the crop stage above (same crop_meta, n_crops, window arithmetic, [-2, size+1]
 * clamp, empty-slot and frame-index handling, same destination) reading uint8 frames [B, H, W, 3]:
 * taps outside the frame contribute raw 0, and every pixel of a filled slot is raw * a[c] + b[c]
 * (as above; swap_rb as above). Empty slots are exact zeros. With a = 1, b = 0 the crops have the
 * bits the fp32 crop stage gives on the same frames converted to float.
 */
int prpe_frame_ingest(const prpe_view_u8* frames, const prpe_view* y, int32_t top, int32_t left, int32_t nh,
                      int32_t nw, const float* a, const float* b, const float* fill, int32_t swap_rb,
                      float* y_amax /* optional */, void* stream);
int prpe_crop_resize_u8(const prpe_view_u8* frames, const float* crop_meta, const int32_t* n_crops,
                        int32_t max_crops, const float* a, const float* b, int32_t swap_rb, float* crops,
                        void* stream);

/*
 * frame_ingest_multi (csrc/ingest_multi.hip; additive to ABI 12): prpe_frame_ingest
 * for a batch whose frames differ in size -- one camera each -- and, with filter = 1, an
 * antialiased downscale. One source frame and where it lands in the model frame:
 */
typedef struct prpe_ingest_src {
  const uint8_t* ptr;        /* device, logical [h, w, 3] */
  int32_t h, w;
  int64_t sh, sw, sc;        /* strides in elements (= bytes) */
  int32_t top, left, nh, nw; /* its region inside H x W (FrameIngest.geometry) */
} prpe_ingest_src;

/*
 * srcs: a HOST array of B frames. It is validated on the host and travels in the kernel arguments,
 * as a, b and fill do: one launch per chunk of at most 32 frames, no upload, no workspace, no
 * allocation, and no pointer to srcs is kept once the call returns. y, a, b, fill, swap_rb, y_amax,
 * the fill outside a frame's region, channel 3 = 0 and the untouched border are prpe_frame_ingest's.
 *
 * filter = 0 (bilinear): for each frame n, y[n] and y_amax[n] have the bytes prpe_frame_ingest
 *   writes for that frame alone with the same region (the arithmetic stated there).
 * filter = 1 (antialias): separable, per axis; stated for x with scale = Ws / nw in fp64, y alike.
 *   scale <= 1 (same size, upscaling): the axis keeps prpe_frame_ingest's two taps and weight, bit
 *   for bit; at nh == Hs and nw == Ws the output still has the bits of torch's u8.float() * a + b.
 *   scale > 1: torch's triangle filter (F.interpolate(mode="bilinear", align_corners=False,
 *   antialias=True); the fp64 weights below are aten's to the bit, checked against the torch build
 *   the tests run on). In fp64:
 *     centre = scale * (j - left + 0.5)
 *     xmin = max((int64)(centre - scale + 0.5), 0),  xmax = min((int64)(centre + scale + 0.5), Ws)
 *     t_k = max(0, 1 - |(k - centre + 0.5) * (1 / scale)|)    for k in [xmin, xmax)
 *     w_k = (float)(t_k / sum t)          (sum: k ascending from 0.0; rounded to fp32 once)
 *   Accumulation in fp32, products then adds, never an fma, every sum ascending from 0.f. A sum
 *   is taken as its first tap plus the weighted differences from it -- prpe_frame_ingest's lerp
 *   v0 + ax * (v1 - v0) carried to n taps -- so a constant window gives the constant exactly
 *   (an all-255 frame is 255 * a + b to the bit), whatever the rounded weights sum to:
 *     h_r = v[r][xmin] + sum_{k > xmin} w_k * (v[r][k] - v[r][xmin])
 *                                         (two-tap x axis: h_r = v0 + ax * (v1 - v0))
 *     raw = h_ymin + sum_{r > ymin} wy_r * (h_r - h_ymin)
 *                                         (two-tap y axis: raw = h_ya + ay * (h_yb - h_ya))
 *     y[.., c] = raw * a[c] + b[c]        as in prpe_frame_ingest.
 *   With weights that sum to 1 this is sum_k w_k v_k; the first tap's own weight is never used.
 *   The order depends on the output pixel alone: a frame's bytes do not depend on B, on its index,
 *   on the chunk it falls in or on its neighbours.
 * -EINVAL, nothing launched (no chunk): a null pointer, B < 1, B != y->n, filter outside {0, 1},
 *   any frame with a null ptr, a side below 1 or above 2^24, or a region that is empty or not inside
 *   H x W; with filter = 1 a frame with h > 32 * nh or w > 32 * nw (8K into 640 is 12);
 *   prpe_frame_ingest's conditions on y. No argument makes the kernel read outside a source frame:
 *   windows are cut to [0, Ws) and two-tap coordinates clamped before they become indices.
 */
int prpe_frame_ingest_multi(const prpe_ingest_src* srcs /* HOST array [B] */, int32_t B, const prpe_view* y,
                            int32_t filter /* 0 bilinear, 1 antialias */, const float* a, const float* b,
                            const float* fill, int32_t swap_rb, float* y_amax /* optional */, void* stream);

/*
 * Face identification: a gallery of enrolled embeddings and a fused cosine top-k search
 * (csrc/gallery.hip). The reference lists face_identification among its tasks
 * (scripts/modify_models.py:331) but has no gallery code; the semantics are this project's.
 *
 * Gallery storage (the search kernel's operand, caller-allocated, 16-byte aligned): fp32
 * [capacity][D] holding the L2-normalised rows, D x 4 bytes per row and nothing else -- the search
 * runs on the fp32-input matrix cores, so the operands are exact fp32 (no bf16 planes, no third
 * plane). norms [capacity] fp32 holds each row's norm before normalisation. D is a multiple of 32
 * in [32, 512].
 *
 * enrol: x [n][D] fp32 with row stride x_row_stride (elements, >= D) -> gallery rows
 *   [row0, row0 + n) and norms [row0, row0 + n): norm = ||x||, row = x / max(norm, 1e-12) with
 *   prpe_l2norm's arithmetic (F.normalize; a zero row stays zero). On the device, no host copy;
 *   no other row is touched, and a row's bytes do not depend on n, row0 or its neighbours.
 *
 * topk: queries [Q][D] fp32 with row stride q_row_stride, normalised inside as above, against
 *   gallery rows [0, G). valid (optional) [G] bytes: a row whose byte is 0 is skipped. k in 1..8.
 *   score(q, g) = the fp32 dot product of the two normalised rows. Candidates are ordered by score
 *   descending, then row ascending; a candidate whose score is not finite (a NaN or infinite
 *   element on either side) is skipped. scores [Q][k] fp32 and rows [Q][k] int32 receive each
 *   query's best k in that order; slots past the number of candidates hold row -1, score -inf.
 *   labels (int64 [G]) and ident (int64 [Q]) go together (both or neither):
 *   ident[q] = labels[rows[q][0]] when rows[q][0] >= 0 and scores[q][0] >= threshold, else -1.
 *   A (query, row) score is the same bits whatever the row's index, G, Q or the other queries of
 *   the launch (one fixed fma order over the columns), so exact duplicate rows tie exactly and
 *   the lower index wins. No atomics: two runs give the same bits.
 *   workspace: >= prpe_gallery_topk_workspace_bytes(Q, G, k) bytes, 256-byte aligned (the
 *   normalised queries and one k-list per query and gallery chunk; the [Q][G] score matrix is never
 *   stored). Concurrent calls on different streams must pass different workspaces.
 * -EINVAL, nothing launched: a null pointer (valid, and labels + ident as a pair, may be null), n,
 *   Q, G or capacity below 1, G above 2^31 - 4097, k outside 1..8, D not a multiple of 32 in
 *   [32, 512], row0 < 0 or row0 + n > capacity, a row stride below D, labels without ident or the
 *   reverse, a misaligned gallery or workspace, a workspace that is too small.
 */
int prpe_gallery_enrol(const float* x, int64_t x_row_stride, int32_t n, int32_t D, float* gallery, float* norms,
                       int32_t capacity, int32_t row0, void* stream);
int64_t prpe_gallery_topk_workspace_bytes(int32_t Q, int32_t G, int32_t k);
int prpe_gallery_topk(const float* queries, int64_t q_row_stride, int32_t Q, int32_t D, const float* gallery,
                      int32_t G, const uint8_t* valid, int32_t k, float* scores, int32_t* rows,
                      const int64_t* labels, float threshold, int64_t* ident, void* workspace,
                      int64_t workspace_bytes, void* stream);

/*
 * The same search for many queries per call (csrc/gallery_wide.hip): a bf16
 * matrix-core pass over the gallery keeps, per query, a set of rows that provably contains the
 * exact top-k; those rows are scored with prpe_gallery_topk's fp32 chain, and a query whose set
 * cannot be proven sufficient is finished by prpe_gallery_topk's own kernels, on the device.
 *
 * Operands, storage and refusals are prpe_gallery_topk's (the gallery is the same fp32 rows: no
 * second copy, no change to enrolment). scores, rows and ident receive the bits prpe_gallery_topk
 * writes for the same call: the order, the skipped non-finite scores, valid, the (-inf, -1) tail
 * and ident's >= threshold included.
 * Premise of that equality: gallery rows [0, G) are prpe_gallery_enrol's output, unit or zero rows
 *   (norm at most 1 up to fp32 rounding) -- what the storage holds by definition. Rows and queries
 *   with NaN or infinite elements are handled as prpe_gallery_topk handles them (skipped).
 * PRPE_GALLERY_WIDE_EPS(D): for such rows, |coarse - exact| <= eps, coarse the bf16 pass's score
 *   and exact the fp32 chain's. With u = 2^-8 the unit roundoff of bf16 round-to-nearest, rounding
 *   both operands moves the real dot product by at most (2u + u^2) |q||g| = 2^-7 + 2^-16
 *   (Cauchy-Schwarz); the fp32 accumulation of the coarse sum (products of two bf16 are exact in
 *   fp32; one ulp, 2^-23, allowed per addition of the matrix core's adder) and of the exact chain
 *   (2^-24 per fma) add less than 3.05 D 2^-24; D 2^-22 covers that, the rounding of the stored
 *   norms and of the bar itself. DESIGN.md 5k has the derivation and the sufficiency argument.
 * route (optional) [Q] bytes: 0 = the filter's certificate held for the query, 1 = the exact
 *   kernels produced its rows.
 * workspace: >= prpe_gallery_topk_wide_workspace_bytes(Q, G, k) bytes, 256-byte aligned; nothing
 *   is allocated, nothing read back, no atomics: two runs give the same bytes. Concurrent calls on
 *   different streams must pass different workspaces.
 * -EINVAL, nothing launched: prpe_gallery_topk's conditions, with this workspace size.
 */
#define PRPE_GALLERY_WIDE_EPS(D) (0.0078125 + 0.0000152587890625 + (double)(D) * (1.0 / 4194304.0))
int64_t prpe_gallery_topk_wide_workspace_bytes(int32_t Q, int32_t G, int32_t k);
int prpe_gallery_topk_wide(const float* queries, int64_t q_row_stride, int32_t Q, int32_t D, const float* gallery,
                           int32_t G, const uint8_t* valid, int32_t k, float* scores, int32_t* rows,
                           const int64_t* labels, float threshold, int64_t* ident, uint8_t* route, void* workspace,
                           int64_t workspace_bytes, void* stream);

/*
 * Per-face identification: face boxes -> 112 x 112 crops in the stem's buffer -> the trunk ->
 * AdaFace -> the gallery, and the join of identities to skeletons (csrc/roi.hip).
 * The reference trains its face branch on 112 x 112 face images through the shared trunk
 * (training/lightning/face_recognition/datamodule.py:41,80) but has no crop stage; the semantics
 * are this project's. crop_meta, n_crops and status are the top-down stage's (above).
 *
 * roi_select: prpe_crop_select with the output size as arguments. Candidate rule, skip rules,
 *   slot order, status bits and crop_meta layout are prpe_crop_select's; the window arithmetic is
 *   its statements in its order (fp32, never fused) with the aspect a = (float)out_w / (float)out_h:
 *   cx = (x1+x2)*0.5, cy = (y1+y2)*0.5; w = x2-x1, h = y2-y1; w > a*h ? h = w/a : w = h*a;
 *   w *= pad, h *= pad; x0 = cx - 0.5*w, y0 = cy - 0.5*h. At out_h = 256, out_w = 192 the output
 *   has prpe_crop_select's bits. -EINVAL as prpe_crop_select, and for out_h or out_w outside
 *   1..4096.
 * roi_resize: frames = a strided view [B, H, W, 3] (any strides); y = a view
 *   [max_crops, out_h, out_w, 4], the interior of any zero-bordered NHWC4 buffer (the stem's
 *   [n, 112+6, 112+8, 4] at rows / columns 3..114, the top-down crop buffer, ...): channel stride 1,
 *   16-byte aligned, the other strides multiples of 4 floats (prpe_frame_ingest's conditions on its
 *   y). The output size is the view's. Slot s < *n_crops: y[s, i, j, 0:3] = the bilinear sample at
 *     (x0 + (j+0.5)*w/out_w - 0.5, y0 + (i+0.5)*h/out_h - 0.5),
 *   taps outside the frame 0 (torch's grid_sample(bilinear, zeros, align_corners=False)), with
 *   prpe_crop_resize's arithmetic: coordinates in fp64, clamped to [-2, size+1] before they become
 *   indices (a NaN coordinate becomes -2: all taps outside), each weight rounded to fp32 once, two
 *   fp32 lerps v00 + ax*(v01 - v00). y[s, i, j, 3] = 0, in the pixel's one 16-byte store. Slots at
 *   or past *n_crops, and slots whose frame index is outside [0, B): zeros. Nothing outside the
 *   view is addressed. Into the top-down crop buffer's interior the bits are prpe_crop_resize's.
 *   y_amax (optional): device [max_crops], zeroed by the caller; y_amax[s] is raised to max|y[s]|
 *   over the slot's interior (one atomicMax on the bit pattern per workgroup; a workgroup never
 *   spans two slots). An empty slot, or a slot whose pixels are all 0, leaves it untouched.
 * roi_resize_u8: the same reading uint8 frames [B, H, W, 3]: taps outside the frame contribute raw
 *   0, and every pixel of a filled slot is raw * a[c] + b[c] (an fp32 multiply, then an add; a, b:
 *   HOST arrays of 3 floats; swap_rb != 0: output channel c reads source channel 2 - c), as
 *   prpe_crop_resize_u8. Empty slots are exact zeros. The bits are those of roi_resize on the
 *   frames converted to float when a = 1, b = 0.
 * -EINVAL, nothing launched: a null pointer (y_amax may be null), frames->c != 3, a frame side
 *   outside 1..2^24, max_crops < 1 or != y->n, y->c != 4, a y that is not channel-contiguous,
 *   16-byte aligned with strides that are multiples of 4, an output side above 4096.
 *
 * face_person_match: identities (of faces) to skeletons (of persons), one wavefront per frame, no
 *   workspace, no atomics: two runs give the same bits.
 *   Persons: crop_meta_p [max_p][8], n_p [1], keypoints [max_p][K][3] = (x, y, score) in frame
 *   pixels (prpe_crop_keypoints). Faces: crop_meta_f [max_f][8], n_f [1], ident [max_f] int64,
 *   score [max_f]. Both lists in the pixels of the same B frames. A frame's persons / faces are the
 *   slots below n_p / n_f with its frame index, in ascending slot order.
 *   Head point of a person: x and y summed over the keypoints k < head_kpts (5 for COCO: nose,
 *   eyes, ears) with score >= kp_thr, in ascending k, in fp32, each sum divided by (float)count;
 *   with count 0 the point (x0 + 0.5f*w, y0 + 0.25f*h) of the person's window.
 *   Face centre: (x0 + 0.5f*w, y0 + 0.5f*h) of the face's window.
 *   A (person, face) pair is eligible when the face centre lies inside the person's window
 *   (cx >= x0, cx <= x0 + w, cy >= y0, cy <= y0 + h; fp32 sums) and its cost is finite.
 *   Cost: dx*dx + dy*dy with dx, dy = head point - face centre (two fp32 products and a sum, never
 *   fused).
 *   Assignment: greedy one-to-one. Repeatedly the eligible pair of least cost among the unmatched
 *   persons and faces is matched, ties to the lower person slot, then the lower face slot, until
 *   no eligible pair is left.
 *   Outputs per person slot: face_slot [max_p] int32 (the matched face's slot, else -1),
 *   person_ident [max_p] int64 (ident of that face, else -1), person_score [max_p] (score of that
 *   face, else -inf). Slots at or past n_p, and slots whose frame index is outside [0, B), get
 *   (-1, -1, -inf). status [B] int32: 1 for a frame with more than 32 persons or more than 32
 *   faces, which gets no matches (the other frames are unaffected), else 0.
 * -EINVAL, nothing launched: a null pointer, max_p, max_f, B or K below 1, head_kpts outside
 *   1..K, a NaN kp_thr.
 */
int prpe_roi_select(const float* dets, const int32_t* counts, int32_t B, int32_t max_det, float score_thr,
                    int32_t max_per_frame, float min_size, float box_scale_x, float box_scale_y, int32_t H,
                    int32_t W, float pad, int32_t out_h, int32_t out_w, int32_t max_crops, float* crop_meta,
                    int32_t* n_crops, int32_t* status, void* stream);
int prpe_roi_resize(const prpe_view* frames, const float* crop_meta, const int32_t* n_crops, int32_t max_crops,
                    const prpe_view* y, float* y_amax /* optional */, void* stream);
int prpe_roi_resize_u8(const prpe_view_u8* frames, const float* crop_meta, const int32_t* n_crops,
                       int32_t max_crops, const float* a, const float* b, int32_t swap_rb, const prpe_view* y,
                       float* y_amax /* optional */, void* stream);
int prpe_face_person_match(const float* crop_meta_p, const int32_t* n_p, int32_t max_p, const float* keypoints,
                           int32_t K, const float* crop_meta_f, const int32_t* n_f, int32_t max_f,
                           const int64_t* ident, const float* score, float kp_thr, int32_t head_kpts, int32_t B,
                           int32_t* face_slot, int64_t* person_ident, float* person_score, int32_t* status,
                           void* stream);

/*
 * Face crops registered to the skeleton (csrc/facealign.hip). The face branch's
 * training images are 112 x 112 faces placed by a similarity transform on the ArcFace landmark
 * positions; the face detector gives no landmarks, the skeleton gives the nose and both eyes.
 *
 * face_align_fit: one thread per person slot s < min(*n_p, max_p). Inputs: the face list
 *   crop_meta_f [max_f][8] and n_f [1], keypoints [max_p][K][3] = (x, y, score) in frame pixels,
 *   person_face [max_p] int32 = prpe_face_person_match's face_slot. Output: warp [max_f][8], zeroed
 *   by the caller (stream-ordered); the call writes only the rows it flags. The match is
 *   one-to-one, so a row has one writer.
 *   warp row: [0] int32 flag (0: use the window of crop_meta; 1: aligned), [1] int32 person slot,
 *   [2..7] = a, b, tx, c, d, ty, the map from the centre of output pixel (i, j) to frame pixels
 *     x = a*(j+0.5) + b*(i+0.5) + tx,   y = c*(j+0.5) + d*(i+0.5) + ty
 *   (pixel k covers [k, k+1), as roi_resize).
 *   The fit, all in fp64 without fused operations: template points q_0..2 = (38.2946, 51.6963),
 *   (73.5318, 51.5014), (56.0252, 71.7366), x times out_w/112 and y times out_h/112 (the factor
 *   formed first), paired with keypoints 2, 1, 0 (COCO right eye, left eye, nose: the subject's
 *   right eye is the viewer's left) = p_0..2. Means (v_0 + v_1 + v_2) / 3; with the centred points
 *   u_i = q_i - mean q, v_i = p_i - mean p, summed in ascending i from 0:
 *     D = sum (u.x*u.x + u.y*u.y), A = sum (u.x*v.x + u.y*v.y) / D, C = sum (u.x*v.y - u.y*v.x) / D,
 *     TX = mean p.x - (A*mean q.x - C*mean q.y), TY = mean p.y - (C*mean q.x + A*mean q.y);
 *   a = d = (float)A, c = (float)C, b = (float)(-C), tx = (float)TX, ty = (float)TY. This is the
 *   least-squares similarity without reflection from template to frame.
 *   The row of face f = person_face[s] is written only when all of these hold, else it stays zero:
 *   0 <= f < min(*n_f, max_f); the three keypoints have score >= kp_thr and finite x, y; the stored
 *   coefficients are finite; the crop's width in frame pixels
 *     size = (float)(sqrt(a*a + c*c) * out_w)         (fp64 on the stored a, c, rounded once)
 *   satisfies scale_lo * w_f <= size <= scale_hi * w_f (exact products in fp64, w_f the face
 *   window's width, both ends inclusive); and the image of the output centre
 *     cx = (float)((a*(out_w/2) + b*(out_h/2)) + tx), cy = (float)((c*(out_w/2) + d*(out_h/2)) + ty)
 *   (fp64 on the stored values, rounded once) lies in the face window: x0 <= cx <= x0 + w_f,
 *   y0 <= cy <= y0 + h_f (fp32 sums, inclusive).
 * -EINVAL, nothing launched: a null pointer, max_f, max_p, out_h or out_w below 1, an output side
 *   above 4096, K < 3, a NaN kp_thr, scale_lo not in (0, scale_hi].
 *
 * roi_warp / roi_warp_u8: roi_resize / roi_resize_u8 with warp [max_crops][8] (device). A slot
 *   whose warp flag is not 1 is resampled from its window exactly as roi_resize does it (the same
 *   statements: the same bits). A slot with flag 1 samples the frame crop_meta[s] names at
 *     sx = (a*(j+0.5) + tx) + b*(i+0.5) - 0.5,   sy = (c*(j+0.5) + ty) + d*(i+0.5) - 0.5
 *   in fp64 from the fp32 coefficients, then as roi_resize: each clamped to [-2, size+1] (NaN
 *   becomes -2), floor, one fp32 rounding per weight, the two fp32 lerps, taps outside the frame 0
 *   and never loaded. Empty slots, channel 3, y_amax, a, b and swap_rb: as roi_resize(_u8). The
 *   launch is roi_resize's: one 128-thread workgroup per (slot, 8 output rows).
 * -EINVAL, nothing launched: a null warp, and whatever roi_resize(_u8) refuses.
 */
int prpe_face_align_fit(const float* crop_meta_f, const int32_t* n_f, int32_t max_f, const int32_t* n_p,
                        int32_t max_p, const float* keypoints, int32_t K, const int32_t* person_face,
                        int32_t out_h, int32_t out_w, float kp_thr, float scale_lo, float scale_hi, float* warp,
                        void* stream);
int prpe_roi_warp(const prpe_view* frames, const float* crop_meta, const int32_t* n_crops, int32_t max_crops,
                  const float* warp, const prpe_view* y, float* y_amax /* optional */, void* stream);
int prpe_roi_warp_u8(const prpe_view_u8* frames, const float* crop_meta, const int32_t* n_crops, int32_t max_crops,
                     const float* warp, const float* a, const float* b, int32_t swap_rb, const prpe_view* y,
                     float* y_amax /* optional */, void* stream);

/*
 * Tracking: persons associated across frames, so that a skeleton keeps its track id and the name
 * once read from its face (csrc/track.hip). The reference has no tracker; the
 * semantics are this project's, after the greedy IoU / OKS trackers of top-down pose demos, with
 * no exp so that a host restatement matches bit for bit. One wavefront per stream walks the
 * stream's frames in order with the track table on chip: one launch, no workspace, no atomics, no
 * host read; two runs give the same bits. Streams are independent of each other and of the slot
 * order of other streams' persons.
 *
 * track_update.
 *   Persons: crop_meta_p [max_p][8], n_p [1], keypoints [max_p][K][3] = (x, y, score) in frame
 *   pixels, person_ident [max_p] int64 and person_score [max_p] as face_person_match leaves them.
 *   A frame's persons are the slots below n_p with its frame index, in ascending slot order. A
 *   person carries an identity when person_ident >= 0 and person_score is finite; its identity
 *   pair is then (person_ident, person_score), else (-1, -inf).
 *   Frames: frame_stream [B] int32 (device) is the stream of frame b; a value outside [0, S): the
 *   frame is not tracked. A stream's frames are taken in ascending b (its time order).
 *   State (the caller's, persistent between calls, T = 32 track slots per stream):
 *   trk_meta [S][32][8] = (id, age, hits as int32 bits; window x0, y0, w, h; the last detection
 *   score), trk_kpts [S][32][K][3], trk_ident [S][32] int64, trk_iscore [S][32], next_id [S]
 *   int32. A free slot has id -1; a track is live when id >= 0. A fresh state is id -1, ident -1,
 *   iscore -inf in every slot and next_id 0 (the other columns may hold anything). The call reads
 *   the state, walks the frames and writes every row back once at the end; a freed slot keeps the
 *   other columns and keypoints it had.
 *   Cost of a (track, person) pair, all fp32, each product, sum and quotient rounded once and
 *   nothing fused:
 *     mode 0 (windows, a = track, b = person):
 *       ix = min(x0a+wa, x0b+wb) - max(x0a, x0b), then ix < 0 ? 0 : ix; iy likewise from y0, h;
 *       inter = ix*iy; uni = wa*ha + wb*hb - inter (left to right); c = 1 - inter/uni.
 *       min(u, v) = v < u ? v : u and max(u, v) = v > u ? v : u (a NaN second operand loses).
 *     mode 1 (skeletons): over the keypoints k in ascending k whose score is >= kp_thr in both
 *       the track and the person: dx, dy = person - track; d_k = (dx*dx + dy*dy) / (area * k2[k])
 *       with area = w*h of the track's window; sum = 0, then sum = sum + d_k;
 *       c = sum / (float)count. count < min_common: the pair is not eligible. k2[k] =
 *       (2 sigma_k)^2 (HOST, K floats). This is the exponent of OKS averaged, not OKS: there is no
 *       exp and no factor 2, and the gate is on this quantity.
 *   A pair is eligible when c is finite and c <= gate.
 *   One frame b of stream s, in this order:
 *   1. More than 32 persons: status[b] = 1 and the frame is skipped whole; the stream's tracks
 *      are neither matched nor aged, its persons get the no-track outputs.
 *   2. Association, greedy and one-to-one over the live tracks and the frame's persons:
 *      repeatedly the eligible pair of least c among the unmatched is matched (-0 equals +0), ties
 *      to the lower track slot, then the lower person slot, until no eligible pair is left.
 *   3. A matched track takes the person's window, keypoints and detection score; age = 0,
 *      hits += 1. A person that carries (ident, s): ident == trk_ident: trk_iscore =
 *      s > trk_iscore ? s : trk_iscore; else if s > trk_iscore: (trk_ident, trk_iscore) =
 *      (ident, s); otherwise, and for a person without an identity, nothing changes.
 *   4. Every unmatched live track: age += 1; age > max_age: freed (id -1, ident -1, iscore -inf).
 *   5. The unmatched persons with detection score >= new_thr, in ascending slot order, each
 *      open a track in the lowest free slot (slots freed in step 4 included): id = next_id[s]++,
 *      hits 1, age 0, the person's window, keypoints, score and identity pair. No free slot:
 *      status[b] |= 2 and the person stays untracked.
 *   status [B] int32: 0, 1 or 2 as above; 0 for a frame that is not tracked.
 *   Outputs per person slot: track_id [max_p] int32, track_hits [max_p] int32, track_ident
 *   [max_p] int64, track_iscore [max_p]: the track's values after the frame's update. Slots at or
 *   past n_p, slots whose frame index is outside [0, B), persons of frames that are not tracked
 *   or skipped, and unmatched persons that opened no track get (-1, 0, -1, -inf).
 * -EINVAL, nothing launched and nothing written: a null pointer, B, S, K or max_p below 1, K above
 *   64, max_p * K * 3 at or above 2^31, mode outside {0, 1}, a NaN gate, kp_thr or new_thr,
 *   min_common outside 1..K, max_age below 0, a k2[k] that is not finite and positive.
 */
int prpe_track_update(const float* crop_meta_p, const int32_t* n_p, int32_t max_p, const float* keypoints,
                      int32_t K, const int64_t* person_ident, const float* person_score,
                      const int32_t* frame_stream, int32_t B, int32_t S, int32_t mode, float gate, float kp_thr,
                      int32_t min_common, const float* k2 /* HOST: K floats */, float new_thr, int32_t max_age,
                      float* trk_meta, float* trk_kpts, int64_t* trk_ident, float* trk_iscore, int32_t* next_id,
                      int32_t* track_id, int32_t* track_hits, int64_t* track_ident, float* track_iscore,
                      int32_t* status, void* stream);

/*
 * Track-level face templates (csrc/tracktemplate.hip; additive to ABI 12): the
 * embeddings of the faces of a track are summed into one template per track, and the template, not
 * the single frame, is what the gallery is asked about. prpe_track_update names a track after its
 * best-scoring frame; a template lets many frames that each stay under the threshold add up, and
 * lets many frames outvote one false accept. The reference has no tracker and no gallery; the
 * semantics are this project's, after the template protocol of AdaFace's video benchmarks (the sum
 * of the un-normalised features, the feature norm being the quality weight).
 *
 * State (the caller's, persistent between calls, beside the tracker's; T = 32 slots per stream,
 *   slot j of stream s belongs to track slot j of trk_meta):
 *   tmpl_owner [S][32] int32: the track id the template belongs to, -1 none;
 *   tmpl_sum [S][32][D] int64: fixed-point sums; tmpl_n [S][32] int32: the faces summed;
 *   tmpl_ident [S][32] int64, tmpl_score [S][32]: the template's name and its score.
 *   Fresh: owner -1, sums 0, n 0, ident -1, score -inf.
 *
 * track_template_update runs after prpe_track_update of the same call, on the same person list
 *   (crop_meta_p [max_p][8], n_p [1]), track_id [max_p] as track_update wrote it, person_face
 *   [max_p] int32 as prpe_face_person_match leaves it, the face list (embeddings [max_f][D] with a
 *   row stride in elements, norms [max_f], n_f [1]; counts are clamped to [0, capacity]),
 *   frame_stream [B], and trk_meta [S][32][8] as track_update left it (read only).
 *   Per slot (s, j), id = the int32 bits of trk_meta[s][j][0]:
 *   1. id < 0: the slot's template is cleared to the fresh values.
 *   2. tmpl_owner != id: the slot was reused; it is cleared, then tmpl_owner = id.
 *   3. Person slot i < n_p is a candidate when its frame b is in [0, B), frame_stream[b] == s,
 *      track_id[i] == id and f = person_face[i] is in [0, n_f). Ids are unique within a stream for
 *      the life of the state, so persons of a track that died earlier in the same call match no
 *      slot and are dropped, and a track that took over a freed slot in the same call starts from
 *      zero. The candidates are taken in ascending i. A candidate contributes when norms[f] is
 *      finite, >= min_norm and < 2^15, all D elements of embeddings[f] are finite, and
 *      tmpl_n < 2^20; otherwise it is skipped whole. A contribution:
 *        tmpl_sum[d] += llrintf(p_d * 2^24), p_d = w * embeddings[f][d] (one fp32 product, nothing
 *        fused; the scaling is exact), w = norms[f] with weight_mode 0 and 1 with weight_mode 1;
 *        tmpl_n += 1.
 *      Embedding rows are unit rows: |p_d| < 2^15, a term is below 2^39 in magnitude and 2^20 of
 *      them stay below 2^59. (A finite element so large that p_d * 2^24 leaves int64 gives an
 *      unspecified sum.) Integer adds commute: the sums equal a host sum exactly, whatever the
 *      order, the split into calls, or the slot order of persons and faces. A face slot that two
 *      persons of a track name contributes twice.
 *   4. A slot that took at least one contribution is DIRTY. The dirty slots in ascending
 *      s * 32 + j form the list: dirty_rows [max_q] int32 (the slot s * 32 + j; -1 at and past
 *      n_dirty), n_dirty [1], dirty_pos [S][32] int32 (the slot's position in the list, -1 for a
 *      slot that is not dirty), queries [max_q][D] fp32 with
 *      queries[r][d] = (float)((double)tmpl_sum[d] * 2^-24), rows at and past n_dirty zero.
 *      max_q >= min(S * 32, max_f) is required: every dirty slot has a face of its own unless two
 *      tracks name one face slot, which prpe_face_person_match never produces. Should it happen
 *      and the list be full, n_dirty = max_q, and the slots past it get their position in
 *      dirty_pos (>= max_q) but no row: they keep their name until they are dirty again.
 *   Two launches in stream order: the sums (one workgroup per slot; a state row is written once,
 *   and only when it is cleared or dirty), then the list. No atomics, no workspace.
 *   The caller then runs prpe_gallery_topk (k = 1, with labels, threshold and ident) on
 *   queries [max_q][D]; it normalises the queries itself.
 *
 * track_template_assign takes that search's ident [max_q] int64 and score [max_q], n_dirty,
 *   dirty_rows and dirty_pos, the state and the person list: for the slot at list position
 *   r < n_dirty, (tmpl_ident, tmpl_score) = (ident[r], score[r]); every other slot keeps what it
 *   had. Per person slot: template_ident [max_p] int64, template_score [max_p], template_faces
 *   [max_p] int32 = the (tmpl_ident, tmpl_score, tmpl_n) after this update of the slot j of its
 *   stream with trk_meta[s][j].id == track_id[i] (a person whose track is live after the call);
 *   every other slot of the person list gets (-1, -inf, 0). One launch: a thread that serves a
 *   person reads the state only of slots that are in no list.
 * -EINVAL, nothing launched and nothing written: a null pointer; B, S, max_p (or, for update,
 *   max_f) below 1; S above 4096 (each of the S workgroups that number the list reads the S * 32
 *   flags of all of them: 2^29 loads at the limit) or max_p above 2^30; update: D not a multiple of 32 in [32, 512],
 *   a row stride below D, max_q below min(S * 32, max_f), weight_mode outside {0, 1}, a NaN
 *   min_norm; assign: max_q below 1.
 */
int prpe_track_template_update(const float* crop_meta_p, const int32_t* n_p, int32_t max_p, const int32_t* track_id,
                               const int32_t* person_face, const float* embeddings, int64_t emb_row_stride,
                               const float* norms, const int32_t* n_f, int32_t max_f, int32_t D,
                               const int32_t* frame_stream, int32_t B, int32_t S, const float* trk_meta,
                               int32_t weight_mode, float min_norm, int32_t* tmpl_owner, int64_t* tmpl_sum,
                               int32_t* tmpl_n, int64_t* tmpl_ident, float* tmpl_score, int32_t* dirty_rows,
                               int32_t* n_dirty, int32_t* dirty_pos, float* queries, int32_t max_q, void* stream);
int prpe_track_template_assign(const float* crop_meta_p, const int32_t* n_p, int32_t max_p, const int32_t* track_id,
                               const int32_t* frame_stream, int32_t B, int32_t S, const float* trk_meta,
                               const int64_t* ident, const float* score, const int32_t* n_dirty,
                               const int32_t* dirty_rows, const int32_t* dirty_pos, int32_t max_q,
                               const int32_t* tmpl_n, int64_t* tmpl_ident, float* tmpl_score, int64_t* template_ident,
                               float* template_score, int32_t* template_faces, void* stream);

/*
 * COCO keypoint evaluation of an epoch's pose records (csrc/cocoeval.hip): what
 * pycocotools' COCOeval(gt, dt, 'keypoints') computes in evaluate(), accumulate() and summarize(),
 * in fp64 and in its operation order, on the records prpe_pose_coco_records left on the device.
 * The library allocates nothing; no atomics: two runs give the same bits. Additive to ABI 12.
 *
 * Fixed sizes: 20 detections kept per image (maxDets), at most 64 ground-truth persons per image,
 * 10 OKS thresholds, 101 recall thresholds, 3 area ranges (all, medium, large), K <= 64.
 *
 * Ground truth (device, CSR over I images in ascending image-id order): gt_start int32 [I+1],
 *   gt_kpts double [G,K,3] (x, y, v), gt_bbox double [G,4] (x, y, w, h), gt_area double [G],
 *   gt_iscrowd uint8 [G], gt_ignore uint8 [G] (iscrowd or num_keypoints == 0). max_gt: the HOST's
 *   maximum of gt_start[i+1] - gt_start[i]; an image whose count is outside 0..64, or whose rows
 *   leave [0, G), is taken as having no ground truth (nothing outside the arrays is addressed).
 * Detections: rec_kpts [n,K,3], rec_meta [n,8] as pose_coco_records leaves them (column 0: image
 *   slot as int32 bits, column 2: score); n = min(*counter, n_max) (counter null: n_max), n_max the
 *   HOST's bound, at most the arrays' capacity. slot_to_img int32 [slots] (device): the image's row
 *   in the ground-truth table; a record whose slot or row is out of range is dropped. The records
 *   of one image must be one contiguous run.
 * HOST constants: sigmas double [K], iou_thrs double [10], area_rngs double [3][2] (lo, hi),
 *   rec_thrs double [101], ascending.
 *
 * coco_kp_match, per image i (one wavefront):
 *   a. The image's records in descending score, stable in record order, NaN last; the first 20.
 *      A detection's area: (max x - min x) * (max y - min y) over its K keypoints.
 *   b. OKS of detection d and ground truth j, vars = (2 sigma)^2, k1 = #(v > 0):
 *      k1 > 0: dx = xd - xg, dy = yd - yg; else with x0 = bx - bw, x1 = bx + 2 bw (y likewise)
 *      dx = max(0, x0 - xd) + max(0, xd - x1); e = (dx^2 + dy^2) / vars / (area_j + 2^-52) / 2;
 *      OKS = sum of exp(-e) over the keypoints with v > 0 (all K when k1 = 0), in ascending k,
 *      over their count.
 *   c. For each area range and threshold t: ground truth j is ignored when gt_ignore or its area
 *      is outside [lo, hi]; the ground truth is walked with the ignored ones last, otherwise in
 *      table order. A detection starts at iou = min(t, 1 - 1e-10), m = none; it skips a matched
 *      ground truth that is no crowd, stops at an ignored one once m is not ignored, skips
 *      oks < iou, else takes (iou, m) = (oks, j). Matched: it takes m's ignore flag and marks m.
 *      Unmatched with its own area outside [lo, hi]: ignored.
 *   d. Slot [i, rank], rank < 20: dt_score float, dt_rec int32 (the record's index, -1 when the
 *      slot is empty), dt_bits uint64: bit a*10+t matched, bit 30+a*10+t ignored, bit 63 the slot
 *      is empty. npig int32 [I,3]: ground truth not ignored per area range. oks_out (optional)
 *      double [I,20,64]: [rank, j], -1 where there is no pair.
 * coco_kp_accumulate: the I*20 slots sorted once by descending score (equal scores in slot order,
 *   empty slots and NaN last); per (a, t) with npig = sum_i npig[i, a] > 0: tp / fp = running
 *   counts of the matched / unmatched slots that are not ignored, rc = tp / npig,
 *   pr = tp / (fp + tp + 2^-52), pr made non-increasing from the back, precision[t, r, a] = pr at
 *   the first slot with rc >= rec_thrs[r] (0 if none), recall[t, a] = the last rc. npig = 0: -1.
 *   precision double [10,101,3], recall double [10,3], stats double [10] = AP, AP50, AP75, APm,
 *   APl, AR, AR50, AR75, ARm, ARl: means of the precision (recall) entries > -1 over all
 *   thresholds (threshold 0 / 5 only for the 50 / 75 ones) of area range 0 (1 for m, 2 for l), summed
 *   in index order; -1 without entries.
 * -EINVAL, nothing launched and nothing written: a null pointer (oks_out and counter may be null;
 *   the record arrays when n_max = 0 and the ground-truth arrays when G = 0 too), I < 1 or
 *   I * 20 >= 2^31, K outside 1..64, G < 0, max_gt outside 0..64, n_max outside 0..2^31-1, a
 *   workspace below *_workspace_bytes, a sigma that is not finite and positive, a NaN threshold or
 *   range bound, rec_thrs that do not ascend strictly.
 */
#define PRPE_COCO_MAX_DETS 20
#define PRPE_COCO_MAX_GT 64
#define PRPE_COCO_IOU_THRS 10
#define PRPE_COCO_REC_THRS 101
#define PRPE_COCO_AREAS 3
int64_t prpe_coco_kp_match_workspace_bytes(int32_t I);
int prpe_coco_kp_match(const float* rec_kpts, const float* rec_meta, const uint64_t* counter /* optional */,
                       int64_t n_max, const int32_t* slot_to_img, int32_t slots, const int32_t* gt_start,
                       const double* gt_kpts, const double* gt_bbox, const double* gt_area,
                       const uint8_t* gt_iscrowd, const uint8_t* gt_ignore, int32_t I, int32_t G, int32_t max_gt,
                       int32_t K, const double* sigmas /* HOST */, const double* iou_thrs /* HOST */,
                       const double* area_rngs /* HOST */, float* dt_score, uint64_t* dt_bits, int32_t* dt_rec,
                       int32_t* npig, double* oks_out /* optional */, void* workspace, int64_t workspace_bytes,
                       void* stream);
int64_t prpe_coco_kp_accumulate_workspace_bytes(int32_t I);
int prpe_coco_kp_accumulate(const float* dt_score, const uint64_t* dt_bits, const int32_t* npig, int32_t I,
                            const double* rec_thrs /* HOST */, double* precision, double* recall, double* stats,
                            void* workspace, int64_t workspace_bytes, void* stream);

/*
 * 1:1 face verification: the scores of all pairs between two sets of enrolled rows, binned into a
 * genuine and an impostor histogram (csrc/pairhist.hip). The score matrix never
 * reaches memory. The reference has no verification code; the semantics are this project's.
 * The library allocates nothing; no host sync. Additive to ABI 12.
 *
 * Operands: a [M][D] and b [N][D], fp32 rows that are ALREADY L2-normalised -- prpe_gallery_enrol's
 *   output, what a gallery stores. Nothing is normalised here (normalising twice is not
 *   bit-idempotent), so a score is the one prpe_gallery_topk compares. Row strides in elements,
 *   >= D and a multiple of 4; a and b 16-byte aligned. D is a multiple of 32 in [32, 512].
 *   a_labels [M] / b_labels [N] int64; a_valid [M] / b_valid [N] optional bytes.
 * Modes: b == NULL is self mode: the pairs (i, j), i < j, of a (b_labels and b_valid must be NULL
 *   too; b_row_stride and N are ignored). Only the upper triangle of score tiles is computed.
 *   Otherwise cross mode: all M x N pairs (a[i], b[j]).
 * score(i, j) = (a0 + a1) + (a2 + a3), a_e the chain acc = fma(x[c], y[c], acc) over the columns c
 *   with c % 4 == e in ascending order: the same bits prpe_gallery_topk gives for those two
 *   normalised rows, whatever the position of the pair, M, N or the mode; score(i, j) == score(j, i).
 * Which pairs count: a row with label < 0 or valid byte 0 takes part in no pair. A pair is genuine
 *   when the two labels are equal, else impostor. A pair whose score is not finite (a NaN or
 *   infinite element on either side) adds 1 to skipped[0] and to no bin.
 * Bins: nbins in {256, 512, 1024, 2048, 4096}, h = nbins / 2,
 *   bin(s) = clamp((int)floorf(s * h) + h, 0, nbins - 1); s * h is exact (h is a power of two; it
 *   is a product and a floor, never fmaf(s, h, h), which would round a tiny negative score up).
 *   With edge_b = (b - h) / h (exact in fp32): for b in 1..nbins-1, s >= edge_b <=> bin(s) >= b, so
 *   the impostor count in bins >= b is exactly the number of pairs an identify at
 *   threshold = edge_b accepts.
 * Output: hist uint64 [2][nbins] (row 0 genuine, row 1 impostor) and skipped uint64 [1] are ADDED
 *   to (64-bit atomic adds), not overwritten: the caller zeroes them, and may chunk a large set or
 *   add several sets into one histogram. Integer adds commute: two runs give the same numbers.
 * -EINVAL, nothing launched and nothing written: a null a, a_labels, hist or skipped; b_labels or
 *   b_valid without b; b without b_labels; M (or, with b, N) below 1 or above 2^24; D not a
 *   multiple of 32 in [32, 512]; nbins outside the list; a row stride below D or not a multiple of
 *   4; a or b not 16-byte aligned. M = 1 in self mode is legal and counts nothing.
 */
int prpe_pair_hist(const float* a, int64_t a_row_stride, int32_t M, const int64_t* a_labels,
                   const uint8_t* a_valid /* optional */, const float* b /* NULL: self mode */,
                   int64_t b_row_stride, int32_t N, const int64_t* b_labels, const uint8_t* b_valid /* optional */,
                   int32_t D, int32_t nbins, uint64_t* hist, uint64_t* skipped, void* stream);

/*
 * Clustering of unlabelled face embeddings: DBSCAN over cosine similarity on enrolled rows, self
 * mode (csrc/facecluster.hip). prpe_pair_hist's GEMM with another epilogue: the
 * score matrix never reaches memory. The reference has no clustering code; the semantics are this
 * project's. The library allocates nothing; no host sync. Additive to ABI 12.
 *
 * Operands: a [N][D], fp32 rows that are ALREADY L2-normalised (prpe_gallery_enrol's output;
 *   nothing is normalised here). Row stride in elements, >= D and a multiple of 4; a 16-byte
 *   aligned; D a multiple of 32 in [32, 512]; 1 <= N <= 2^24, as for prpe_pair_hist. valid [N]:
 *   optional bytes; a row with valid byte 0 takes part in nothing. Labels play no role.
 * score(i, j): prpe_pair_hist's and prpe_gallery_topk's bits, (a0 + a1) + (a2 + a3), a_e the chain
 *   acc = fma(x[c], y[c], acc) over the columns c with c % 4 == e in ascending order.
 * Neighbours: i and j are neighbours when i != j, both rows take part, the score is finite and
 *   score(i, j) >= threshold (fp32 compare; equality accepts, as prpe_gallery_topk's ident does).
 *   A NaN or infinite score is no neighbour and is counted nowhere.
 * degree[i]: the number of neighbours of i (0 for a row that takes no part). A row is CORE when
 *   degree[i] + 1 >= min_samples (the row counts itself). With min_samples == 1 every row that
 *   takes part is core and the clusters are the connected components (single linkage).
 * Clusters: two core rows that are neighbours are in one cluster, transitively.
 * Border: a row that takes part, is not core and has at least one core neighbour joins the cluster
 *   of the core neighbour with the highest score, the lowest row on ties. (Textbook DBSCAN leaves
 *   this to visiting order; here two runs must agree.) Every other row that takes part is noise.
 * Outputs, all caller-allocated device memory:
 *   root [N] int32: the lowest core row of the row's cluster; -1 for noise and left-out rows.
 *   kind [N] uint8: 0 left out, 1 noise, 2 border, 3 core.
 *   degree [N] int32.
 *   cluster [N] int32: compact ids 0 .. C-1, ascending with the cluster's root; -1 where root is.
 *   n_clusters [1] int32: the true C, also when it exceeds max_clusters.
 *   sizes [max_clusters] int32: core and border members per cluster.
 *   sums [max_clusters][D] int64: per cluster and column the sum over its members of
 *     llrintf(a[i][d] * 2^32) (the product is exact). Integer adds commute: the sums equal a host
 *     sum exactly on every run; |element| <= 1 and N <= 2^24 bound a sum by 2^56. The sums of a
 *     cluster that holds a NaN or infinite element are unspecified.
 *   centroids [max_clusters][D] fp32: (float)((double)sums * 2^-32), not normalised.
 *   Clusters with id >= max_clusters keep their ids in cluster but get no size, sum or centroid;
 *   the rows of sizes, sums and centroids past min(C, max_clusters) are left untouched.
 * Every output is a function of the inputs alone: two runs, any grid and any tile order give the
 *   same bits.
 * Stages (each needs the previous one's outputs, in stream order):
 *   prpe_pair_degree  overwrites degree.
 *   prpe_pair_link    initialises the workspace (best [N] uint64, then parent [N] int32; at least
 *     prpe_face_cluster_workspace_bytes(N) bytes, 256-byte aligned) and links: the core rows of a
 *     cluster end under one root in a union-find (parent[x] <= x, hooks by compare-and-swap, the
 *     root the lowest core row), a border candidate's best core neighbour in
 *     best = image(score) << 32 | (0xFFFFFFFF - row), image the order-preserving uint32 of the score.
 *   prpe_cluster_finish  reads degree and the workspace; writes root, kind, cluster, n_clusters and
 *     sizes[0 .. min(C, max_clusters)).
 *   prpe_cluster_centroids  reads cluster and n_clusters; writes sums and centroids
 *     [0 .. min(C, max_clusters)).
 * -EINVAL, nothing launched and nothing written: what prpe_pair_hist refuses of a, its stride, N
 *   and D; min_samples < 1; a threshold that is not finite; max_clusters < 1; a null degree or
 *   output; a workspace that is null, too small or not 256-byte aligned.
 *   prpe_face_cluster_workspace_bytes returns -EINVAL for N outside [1, 2^24].
 */
int64_t prpe_face_cluster_workspace_bytes(int32_t N);
int prpe_pair_degree(const float* a, int64_t a_row_stride, int32_t N, const uint8_t* valid /* optional */, int32_t D,
                     float threshold, int32_t* degree, void* stream);
int prpe_pair_link(const float* a, int64_t a_row_stride, int32_t N, const uint8_t* valid /* optional */, int32_t D,
                   float threshold, int32_t min_samples, const int32_t* degree, void* workspace,
                   int64_t workspace_bytes, void* stream);
int prpe_cluster_finish(int32_t N, const uint8_t* valid /* optional */, int32_t min_samples, const int32_t* degree,
                        const void* workspace, int64_t workspace_bytes, int32_t* root, uint8_t* kind,
                        int32_t* cluster, int32_t* n_clusters, int32_t max_clusters, int32_t* sizes, void* stream);
int prpe_cluster_centroids(const float* a, int64_t a_row_stride, int32_t N, int32_t D, const int32_t* cluster,
                           const int32_t* n_clusters, int32_t max_clusters, int64_t* sums, float* centroids,
                           void* stream);

/*
 * Open-set 1:N identification evaluation: per probe the best enrolled row of its own label (its
 * mate), the best row of any other label, the rank of the first mate, and from these the
 * histograms behind DIR / FNIR / FPIR and the CMC (csrc/identeval.hip).
 * prpe_pair_hist's GEMM with a third epilogue: the score matrix never reaches memory. The reference
 * has no such code; the semantics are this project's. The library allocates nothing; no host
 * sync. Additive to ABI 12.
 *
 * Operands: as for prpe_pair_hist. Probes a [M][D] and gallery b [N][D], fp32 rows that are ALREADY
 *   L2-normalised (prpe_gallery_enrol's output). Row strides in elements, >= D and a multiple of 4;
 *   a and b 16-byte aligned; D a multiple of 32 in [32, 512]; 1 <= M, N <= 2^24. a_labels [M] /
 *   b_labels [N] int64; a_valid [M] / b_valid [N] optional bytes. The uint64 arrays are 8-byte
 *   aligned.
 * score(i, j): prpe_pair_hist's, prpe_pair_link's and prpe_gallery_topk's bits, (a0 + a1) + (a2 + a3),
 *   a_e the chain acc = fma(x[c], y[c], acc) over the columns c with c % 4 == e in ascending order.
 * Which rows take part: a probe when its valid byte is non-zero and its label >= 0; a gallery row
 *   when its valid byte is non-zero (its label is only compared, as prpe_gallery_topk does: a
 *   negative one equals no probe's). A (probe, row) combination of rows that take part is a
 *   candidate when its score is finite; otherwise it adds 1 to skipped[0].
 * Modes: b != NULL is cross mode: every probe against every gallery row; candidate row j of b has
 *   the number b_row0 + j (b_row0 >= 0, b_row0 + N <= 2^31 - 1), so a gallery may be passed in
 *   several row ranges into the same outputs. b == NULL is self mode, leave-one-out on one
 *   labelled set: every row of a is a probe against all other rows (i != j); b_labels and b_valid
 *   must be NULL and b_row0 0 (b_row_stride and N are ignored). Only the upper triangle of score
 *   tiles is computed: a pair (i, j), i < j, serves probe i with row j and probe j with row i
 *   (score(i, j) == score(j, i)). skipped counts both directions. M = 1 is legal and finds nothing.
 * Order: the candidates of a probe are ordered as prpe_gallery_topk orders them, score descending,
 *   then row ascending, by one key per candidate:
 *     key = image(score) << 32 | (0xFFFFFFFF - row),
 *   image(s) = u ^ (u >> 31 ? 0xFFFFFFFF : 0x80000000) with u the bits of s after -0 became +0.
 *   A larger key is an earlier candidate; no candidate has key 0, which means "none".
 * prpe_ident_best (pass 1): mate_key[i] = the largest key over the candidates of probe i whose label
 *   equals the probe's, non_key[i] = the largest over the others. 64-bit atomic maxima into the
 *   caller-zeroed [M] arrays (one per probe row and tile side, after a reduction in registers and
 *   LDS); the slots of probes that take no part are not written. A max commutes: two runs, any
 *   grid and any split of the gallery give the same bits. skipped [1] is ADDED to.
 * prpe_ident_rank (pass 2): the same product, reading mate_key (complete: of the whole gallery).
 *   rank_minus_1[i], caller-zeroed int32 [M], is ADDED the number of non-mate candidates of probe i
 *   whose key is greater than mate_key[i]; a probe without a mate adds nothing. The rank counts
 *   gallery ROWS, not identities: rank r means the first mate is the r-th entry of an unbounded
 *   search.
 * prpe_ident_finish: one small launch over the M probes. Writes
 *     mate_score, non_score fp32 [M] and mate_row, non_row int32 [M]: the keys decoded (-0 reads
 *       +0); -inf and -1 for an empty slot and for a probe that takes no part;
 *     rank int32 [M]: 0 when the probe takes no part or has no mate, else rank_minus_1 + 1.
 *   and ADDS (64-bit atomic adds; the caller zeroes them, and may pass the probes in several calls)
 *     hist uint64 [3][nbins], prpe_pair_hist's bins (nbins in {256 .. 4096}, h = nbins / 2,
 *       bin(s) = clamp((int)floorf(s * h) + h, 0, nbins - 1)):
 *       row 0: the mated probes with mate_key > non_key (rank 1), binned by mate_score;
 *       row 1: the mated probes with rank > 1, binned by non_score (the wrong label an identify
 *              would return);
 *       row 2: the probes that take part and have no mate (strangers to the gallery) but at least
 *              one candidate, binned by non_score.
 *       Bin edges are exact in fp32, so for every edge t = edge_b the sums of rows 0, 1 and 2 over
 *       the bins >= b are EXACTLY the probes for which an identify at threshold t returns the right
 *       label, a wrong label, and any label for a stranger.
 *     rank_hist uint64 [PRPE_IDENT_RANKS + 1]: every mated probe in slot min(rank, R + 1) - 1.
 *     counts uint64 [4]: mated probes; non-mated probes (those without any candidate included);
 *       probes left out; non-mated probes without any candidate. [0] + [1] + [2] == M.
 *   rank_minus_1 is optional (pass 2 not run): then rank is 1 for mate_key > non_key, -1 for the
 *   other mated probes, rank_hist must be NULL and is not written.
 * -EINVAL, nothing launched and nothing written: a null a, a_labels, mate_key, non_key, skipped,
 *   rank_minus_1 (rank) or output; b_labels, b_valid or a non-zero b_row0 without b; b without
 *   b_labels; M (or, with b, N) below 1 or above 2^24; b_row0 < 0 or b_row0 + N > 2^31 - 1; D not a
 *   multiple of 32 in [32, 512]; a row stride below D or not a multiple of 4; a or b not 16-byte
 *   aligned; a uint64 array not 8-byte aligned; nbins outside the list; rank_hist without
 *   rank_minus_1 or rank_minus_1 without rank_hist.
 */
#define PRPE_IDENT_RANKS 64
int prpe_ident_best(const float* a, int64_t a_row_stride, int32_t M, const int64_t* a_labels,
                    const uint8_t* a_valid /* optional */, const float* b /* NULL: self mode */, int64_t b_row_stride,
                    int32_t N, const int64_t* b_labels, const uint8_t* b_valid /* optional */, int32_t b_row0,
                    int32_t D, uint64_t* mate_key, uint64_t* non_key, uint64_t* skipped, void* stream);
int prpe_ident_rank(const float* a, int64_t a_row_stride, int32_t M, const int64_t* a_labels,
                    const uint8_t* a_valid /* optional */, const float* b /* NULL: self mode */, int64_t b_row_stride,
                    int32_t N, const int64_t* b_labels, const uint8_t* b_valid /* optional */, int32_t b_row0,
                    int32_t D, const uint64_t* mate_key, int32_t* rank_minus_1, void* stream);
int prpe_ident_finish(int32_t M, const int64_t* a_labels, const uint8_t* a_valid /* optional */,
                      const uint64_t* mate_key, const uint64_t* non_key, const int32_t* rank_minus_1 /* optional */,
                      int32_t nbins, float* mate_score, int32_t* mate_row, float* non_score, int32_t* non_row,
                      int32_t* rank, uint64_t* hist, uint64_t* rank_hist /* with rank_minus_1 */, uint64_t* counts,
                      void* stream);

/*
 * NV12 frames in (csrc/nv12.hip; additive to ABI 12): what a hardware video decoder
 * hands over -- a full-resolution luma plane, a half-resolution plane of interleaved chroma pairs
 * and a row pitch wider than the picture -- read by the stem and crop stages themselves, with no
 * conversion pass and no RGB copy in front of them. The reference reads decoded images only; the
 * semantics are this project's.
 *
 * The source. Odd h and w are legal: the chroma plane has the rounded-up size. y and uv may be two
 * allocations, or two views of one decoder surface (the chroma rows following the aligned luma
 * rows at the same pitch). Bytes between w and the pitch, and rows below h, are never read.
 */
typedef struct prpe_nv12 {
  const uint8_t* y;     /* device, logical [n, h, w], element stride 1 along w */
  const uint8_t* uv;    /* device, logical [n, (h+1)/2, (w+1)/2, 2] = (U, V), 2 contiguous bytes per pair */
  int32_t n, h, w;
  int64_t y_sn, y_sh;   /* bytes; y_sh >= w (the decoder's pitch) */
  int64_t uv_sn, uv_sh; /* bytes; uv_sh >= 2 * ((w+1)/2) */
} prpe_nv12;

/*
 * The conversion: one rule, in integers, so that a host restatement is exact.
 *   Chroma is replicated: pixel (i, j) takes the pair at (i >> 1, j >> 1) (nearest siting).
 *   coef = (y_off, cy, crv, cgu, cgv, cbu): a HOST array of 6 int32; it travels in the kernel
 *   arguments, as a, b and fill do.
 *     C = Y - y_off;  D = U - 128;  E = V - 128
 *     R = clamp(floor((cy*C + crv*E + 128) / 256), 0, 255)
 *     G = clamp(floor((cy*C - cgu*D - cgv*E + 128) / 256), 0, 255)
 *     B = clamp(floor((cy*C + cbu*D + 128) / 256), 0, 255)
 *   floor on a negative numerator is an arithmetic shift right by 8. y_off must be in [0, 255] and
 *   every other entry in [0, 4096]; the sums then stay far inside 32 bits (below 2^22).
 *   The named tables are round(256 x) of the real matrices (prpe/nv12.py):
 *     bt601 limited (16, 298, 409, 100, 208, 516)     bt601 full (0, 256, 359, 88, 183, 454)
 *     bt709 limited (16, 298, 459,  55, 136, 541)     bt709 full (0, 256, 403, 48, 120, 475)
 *   with crv = 2(1 - Kr), cbu = 2(1 - Kb), cgu = cbu Kb / Kg, cgv = crv Kr / Kg, Kg = 1 - Kr - Kb;
 *   limited range scales luma by 255/219 and chroma by 255/224.
 *
 * The one property everything is held to: a converted tap is a uint8 value, so each fused entry
 * point below has, bit for bit, the output of its _u8 twin run on the frames prpe_nv12_to_rgb
 * writes -- the same coordinates, weights, lerps, affine, fill, clamp and y_amax. No new floating-
 * point rule exists; the new arithmetic is the integer conversion alone. The fused entry points
 * have no swap_rb: output channels 0, 1, 2 are R, G, B, which is what the u8 route gives on a
 * conversion made in the ingest's own channel order. A tap outside the frame in a crop stage is raw
 * 0 in all three channels (as in the _u8 kernels), not the conversion of a zero triple.
 *
 * All five are stream-ordered, allocate nothing and decide every refusal before the launch.
 *
 * nv12_to_rgb: out, packed uint8 [n, h, w, 3] with row stride osh and frame stride osn in bytes
 *   (osh >= 3 w); swap_rb != 0 writes B, G, R. The unfused route and the yardstick of the others.
 *   8-byte loads and stores are used where the planes, out and all their strides are 8-byte
 *   aligned; any alignment is legal. Padding bytes of out are never written.
 * frame_ingest_nv12: prpe_frame_ingest (y, region, a, b, fill, y_amax as there) on converted taps.
 * crop_resize_nv12, roi_resize_nv12, roi_warp_nv12: prpe_crop_resize_u8, prpe_roi_resize_u8 and
 *   prpe_roi_warp_u8 on converted taps; crop_meta's windows are in the pixels of these frames.
 * -EINVAL, nothing launched: every refusal of the respective twin; a null src, coef or plane; n
 *   below 1; a side below 1 or above 2^24; a pitch below the row (y_sh < w,
 *   uv_sh < 2 * ((w+1)/2), osh < 3 w); an odd uv pointer, uv_sn or uv_sh (a pair is one aligned
 *   16-bit load); a coefficient out of range; n != y->n for the ingest; a null out. No argument
 *   makes a kernel read outside [0, h) x [0, w) of the luma plane or outside the rounded-up chroma
 *   plane: indices are clamped or bounds-tested before they are used, as in the twins.
 */
int prpe_nv12_to_rgb(const prpe_nv12* src, const int32_t* coef /* HOST: 6 */, int32_t swap_rb, uint8_t* out,
                     int64_t osn, int64_t osh, void* stream);
int prpe_frame_ingest_nv12(const prpe_nv12* src, const int32_t* coef /* HOST: 6 */, const prpe_view* y, int32_t top,
                           int32_t left, int32_t nh, int32_t nw, const float* a, const float* b, const float* fill,
                           float* y_amax /* optional */, void* stream);
int prpe_crop_resize_nv12(const prpe_nv12* src, const int32_t* coef /* HOST: 6 */, const float* crop_meta,
                          const int32_t* n_crops, int32_t max_crops, const float* a, const float* b, float* crops,
                          void* stream);
int prpe_roi_resize_nv12(const prpe_nv12* src, const int32_t* coef /* HOST: 6 */, const float* crop_meta,
                         const int32_t* n_crops, int32_t max_crops, const prpe_view* y, const float* a,
                         const float* b, float* y_amax /* optional */, void* stream);
int prpe_roi_warp_nv12(const prpe_nv12* src, const int32_t* coef /* HOST: 6 */, const float* crop_meta,
                       const int32_t* n_crops, int32_t max_crops, const float* warp, const prpe_view* y,
                       const float* a, const float* b, float* y_amax /* optional */, void* stream);

/*
 * Annotated frames out (csrc/annotate.hip; additive to ABI 12): skeletons, person
 * boxes and face redaction painted IN PLACE into the surface that goes to the encoder or the
 * display, from the device arrays the crop, pose, face and tracking stages leave. The reference has
 * no drawing code (a TODO in its callbacks.py); the semantics are this project's, chosen so that a
 * host restatement is exact: one fp32 rounding per coordinate, everything after it in integers.
 *
 * The surface. prpe_annotate_nv12 writes the two planes its prpe_nv12 names: the struct's const
 * is the reader's, the pointers are written through. prpe_annotate_u8 writes a prpe_view_u8 [B, H, W, 3]
 * with any strides. Sides are 1..16384. Bytes between w and the pitch and rows below h are never
 * written; a pixel no primitive covers is neither read nor written.
 *
 * Inputs, all device arrays read on the device except limbs:
 *   crop_meta_p [max_p][8], n_p [1], keypoints [max_p][K][3] = (x, y, score), 1 <= K <= 64;
 *   person_colour [max_p] int32: palette index, negative = the person is not drawn;
 *   crop_meta_f [max_f][8], n_f [1], face_mode [max_f] int32 (1 pixelate, 2 fill, anything else
 *   leave), face_colour [max_f] int32;
 *   palette [n_colours][4] uint8, 4-byte aligned: (Y, U, V, 0) for the NV12 twin, (c0, c1, c2, 0)
 *   for the u8 twin; a colour index is reduced modulo n_colours on the device (a negative
 *   face_colour to the non-negative residue);
 *   limbs: HOST, n_limbs <= 32 pairs of keypoint indices; it travels in the kernel arguments.
 *   max_p and max_f are 0..2^20; with a capacity of 0 that list's pointers may be null.
 *   A slot at or past its count (clamped to [0, capacity]) or with a frame index outside [0, B)
 *   draws nothing.
 * Scalars: box_t 0..16 (outline thickness; 0 = no boxes), limb_r and kp_r 0..16 (radii in pixels),
 *   kp_thr, cell (even, 2..64), sx and sy (finite, positive: list coordinates -> surface pixels).
 *
 * Float to integer, the only floating point: a coordinate is q = rintf(v * s), one fp32 multiply,
 *   then round half to even. A window (x0, y0, w, h = crop_meta[2..5]) is X0 = rintf(x0 * sx),
 *   X1 = rintf((x0 + w) * sx) (the fp32 sum first, then the multiply; no contraction), Y likewise.
 *   A primitive is skipped when one of its products is not finite or one of its rounded
 *   coordinates is outside [-4096, 20479]; a window also when it is empty (X1 <= X0 or Y1 <= Y0).
 *   Keypoint j counts when score >= kp_thr (a NaN score does not) and its two coordinates pass; a
 *   limb needs both of its ends.
 * Coverage, exact integers on pixel coordinates p = (x, y), 0 <= x < w, 0 <= y < h:
 *   disc (c, r):       |p - c|^2 <= r^2
 *   segment (a, b, r): with d = b - a, L2 = d.d: |p - a|^2 <= r^2, or |p - b|^2 <= r^2, or
 *                      (L2 > 0 and 0 <= (p - a).d <= L2 and cross(d, p - a)^2 <= r^2 L2): round
 *                      caps; L2 = 0 is a disc.
 *   box outline:       inside [X0, X1) x [Y0, Y1) and not inside that rectangle shrunk by box_t on
 *                      every side (a shrunk rectangle that is empty leaves the whole window).
 *   Widths: a pixel is in [0, 16383] and a coordinate in [-4096, 20479], so every component of
 *   p - a is within +-20479 < 2^15 and of d within +-24575 < 2^15. |p - a|^2, L2 and (p - a).d
 *   are sums of two products below 2^30 in magnitude each, so below 2^31: they fit int32 (the
 *   largest, 2 * 24575^2 = 1 207 861 250). cross(d, p - a) is bounded by 2 * 24575 * 20479 < 2^30.1;
 *   it and its square (< 2^60.1) are formed in int64; r^2 L2 <= 256 * 2^31 = 2^39. Nothing
 *   approaches 2^63.
 * Priority: a pixel takes the highest layer that covers it, face redaction < boxes < limbs <
 *   keypoint discs; inside a layer the lowest slot wins. A person's layers take palette
 *   [person_colour]. Every painted byte is written exactly once; two runs give the same bytes.
 * Redaction: a face's window clipped to the frame; overlapping faces by lowest slot. Mode 2 fills
 *   with palette[face_colour]. Mode 1 pixelates: block side c = max(cell, 2 * ((side + 31) / 32)),
 *   side = max(X1 - X0, Y1 - Y0) unclipped (at most 17 blocks per side); blocks anchored at
 *   (X0 & ~1, Y0 & ~1); a block's value per channel is (sum + n / 2) / n over the block's samples
 *   inside the frame (not clipped to the window). On NV12 luma is averaged over the block's luma
 *   pixels and U, V over its chroma pairs; c and the anchor are even, so a pair lies in one block.
 *   The means are taken by the first launch, from the surface as it is before anything is
 *   painted, into means [max_f][17][17][4] uint8 (caller's, 4-byte aligned), and applied by the
 *   second; stream order makes the in-place update safe.
 * NV12 chroma: the pair (ci, cj) is painted exactly when luma pixel (2 ci, 2 cj) is, by the same
 *   primitive's palette entry or block. So the painted luma pixels are the painted pixels of the
 *   u8 twin on the same inputs.
 * Workspaces: table, 16-byte aligned, at least prpe_annotate_table_bytes(max_p, max_f, K, n_limbs)
 *   bytes (the integer primitives and their bounding boxes), and means. The library allocates
 *   nothing and reads nothing back. prpe_annotate_geometry: out [4] = (tile h, tile w, super-tile
 *   h, super-tile w), the paint launch's partition of the frame.
 * -EINVAL, nothing launched and nothing written: a null dst, args, plane, palette, or list pointer
 *   of a list with capacity > 0 (means included, for max_f > 0); limbs null with n_limbs > 0; a
 *   side outside 1..16384 or n < 1; the plane and pitch refusals of the NV12 block above; c != 3
 *   for the u8 twin; K outside 1..64; n_limbs outside 0..32 or a limb index outside [0, K); max_p
 *   or max_f outside 0..2^20; box_t, limb_r or kp_r outside 0..16; cell odd or outside 2..64;
 *   n_colours < 1; sx or sy not finite or not positive; a NaN kp_thr; a palette or means pointer
 *   that is not 4-byte aligned; a table that is null, not 16-byte aligned or too small.
 *   prpe_annotate_table_bytes returns -EINVAL for sizes outside the ranges above.
 *   With max_p = max_f = 0 a call is legal and launches nothing.
 */
typedef struct prpe_annotate_args {
  const float* crop_meta_p; const int32_t* n_p; const float* keypoints; const int32_t* person_colour;
  const float* crop_meta_f; const int32_t* n_f; const int32_t* face_mode; const int32_t* face_colour;
  const uint8_t* palette; const int32_t* limbs /* HOST: 2 * n_limbs */;
  void* table; uint8_t* means;
  int64_t table_bytes;
  int32_t max_p, K, max_f, n_colours, n_limbs;
  int32_t box_t, limb_r, kp_r, cell;
  float kp_thr, sx, sy;
} prpe_annotate_args;
void prpe_annotate_geometry(int32_t* out /* HOST: 4 */);
int64_t prpe_annotate_table_bytes(int32_t max_p, int32_t max_f, int32_t K, int32_t n_limbs);
int prpe_annotate_nv12(const prpe_nv12* dst, const prpe_annotate_args* args, void* stream);
int prpe_annotate_u8(const prpe_view_u8* dst, const prpe_annotate_args* args, void* stream);

/* ABI version / build info. prpe_source_hash: sha256 (hex) of the sources the library was built
 * from (csrc/*.hip, csrc/*.h, include/prpe.h; computed by build.py), so a host binding can refuse
 * a library built from other sources than the ones beside it. */
int prpe_abi_version(void);
const char* prpe_build_info(void);
const char* prpe_source_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* PRPE_H_ */
