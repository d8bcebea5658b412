/*
 * pds_hip.h -- C ABI of libpds_hip.so: the MI355X (gfx950) implementation of the
 * Practical Deep Stereo cost-volume hot path (Matching -> Regularization -> SubpixelMap).
 *
 * The reference has no FFI on this path: the seam is Python constructor injection
 * (reference practical_deep_stereo/network.py:17-24) and the modules are torch.nn code.
 * The entry points below are therefore what a ctypes/cffi binding of each reference
 * module's forward would call; every prototype cites the reference code it replaces.
 * INTEGRATION.md shows the reference-side stub.
 *
 * Conventions (all entry points):
 *  - plain C: raw device pointers, ints, one opaque stream handle (a hipStream_t).
 *    No torch types.  All tensors are contiguous fp32, NCHW / NCDHW like the reference.
 *  - the library never allocates, frees or synchronises: every buffer (inputs, outputs,
 *    workspace, packed weights) belongs to the caller; all work is enqueued on `stream`;
 *    calls are re-entrant and hipGraph-capturable.
 *  - return value 0 = enqueued; non-zero = error (negative: bad argument, positive:
 *    hipError_t).  pds_last_error() gives a thread-local message.  Nothing throws.
 *  - `weights_resident` (the forward entry points that re-lay weights out): pass 0 unless this
 *    very workspace was last used by the same entry point with the same shapes and the same
 *    parameter VALUES; then 1 skips the weight re-layout launches (the packed weights a module
 *    owns are immutable between optimizer steps).  The Python mirror tracks this
 *    through the parameters' version counters.
 *  - argument validation that the reference does in Python (the ValueErrors of
 *    estimator.py:34-41, network.py:28-31) stays in the Python mirror.
 */
#ifndef PDS_HIP_H
#define PDS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDS_ABI_VERSION 7

typedef void* pds_stream_t; /* hipStream_t */

int pds_abi_version(void);
const char* pds_last_error(void);

/* ABI v5.  Non-finite InstanceNorm statistics.  The reference propagates NaN / inf silently (network_blocks.py:47-85
 * have no checks); here every statistics kernel that finds a group whose mean or variance is not finite (a NaN / inf
 * in the caller's tensors or parameters, or an overflow) bumps a counter in host-mapped memory, so a caller can
 * tell "garbage in" from a number WITHOUT a device synchronisation in the hot path.  Returns the count reported by
 * kernels that have completed so far (all devices of the process; synchronise the stream first for an exact answer)
 * and resets it when `reset` is non-zero; -1 when the counter could not be set up. */
long long pds_nonfinite_statistics(int reset);

/* ABI v5.  Launch probe (measurement only; bench.py's roofline): times named kernels IN SITU -- inside whatever
 * sequence of launches the caller enqueues -- with a HIP event pair on the launch stream around each of them, instead
 * of a micro-benchmark of the isolated kernel.  pds_probe_begin arms the probe for launches whose name contains
 * `kernel` ("conv2d_x3", "conv2d_t8w"), at most `capacity` of them (<= 256; events are created on first use and
 * re-used).  Names of the 2-D convolution launchers: "conv2d_x3<fp16>", "conv2d_x3<bf16>", "conv2d_t8w",
 * "conv2d_t8<tile>", "conv2d_wino<4r>", "conv2d_wino<6r>", "conv2d_wino16", "conv2d_mfma<mb4>", "conv2d_mfma<mb1>",
 * "conv_direct<2d>" ("conv_direct<3d>" for kernel depth 3); the match is by substring, so "conv2d_wino" counts all three
 * Winograd forms and "conv_direct" the transposed "deconv_direct" as well.  Names of the weight-gradient launchers of the
 * backward pass (none contains another): "wgrad2d_mfma<mb4>", "wgrad2d_mfma<mb4,2src>", "wgrad2d_mfma<mb4,partial>",
 * "wgrad2d_mfma<mb1>", "wgrad2d_mfma<mb1,2src>", "wgrad2d_x3", "wgrad3d_mfma<pair>", "wgrad3d_mfma<pair,2src>",
 * "wgrad3d_mfma<tap>", "wgrad3d_mfma<tap,2src>", "wgrad3d_s2_mfma<conv>", "wgrad3d_s2_mfma<deconv>", "wgrad3d_s2r<conv>",
 * "wgrad3d_s2r<deconv>", "wgrad_up_full_mfma", the VALU fallbacks "bwd_weight<conv>" / "bwd_weight<deconv>", and the
 * reductions that follow them, "wgrad_reduce_f32" (every matrix-pipe form) and "weight_reduce" (the fallbacks).
 * pds_probe_end disarms it, waits for the recorded events and writes the durations in launch order
 * (milliseconds) and the launch grids (workgroups) to ms[] / workgroups[] (either may be NULL); returns the number of
 * launches recorded, or a negative error code.  Not thread-safe and not for production paths: events between
 * launches serialise them. */
int pds_probe_begin(const char* kernel, int capacity);
int pds_probe_end(float* ms, int* workgroups, int capacity);

/* ABI v6.  Measurement only: the inner levels of the Regularization hourglass (regularization.py:22-26, 48-52: the
 * layers the K-split kernel serves) run as ONE persistent launch whose workgroups walk the layer list (conv3d_ks.hip:
 * conv3d_ks_chain_kernel).  Synchronises the device and writes, for every layer of the LAST such launch of this
 * process, the time at which it was complete (InstanceNorm folded) in ticks of the 100 MHz device clock since the
 * first ticket of the launch was drawn; returns the number of layers (0: no such launch yet) or a negative error code.
 * (The chain kernel never hangs the GPU: a workgroup whose producer layer does not report within 2 s stops waiting and
 * adds 2^20 to the counter behind pds_nonfinite_statistics -- the results of that launch are then garbage, and visible as such.) */
int pds_debug_chain_stamps(unsigned* ticks, int capacity);

/* ------------------------------------------------------------------------------------
 * Layer parameters in the reference's own (PyTorch) layouts.
 *   conv   weight [Cout, Cin, kD, kH, kW]  (Conv2d: kD == 1)   network_blocks.py:9-24
 *   deconv weight [Cin, Cout, kD, kH, kW]                      network_blocks.py:37-44, 75-85
 *   gamma/beta: InstanceNorm affine (NULL for a bare conv)     network_blocks.py:58,72,85
 * ---------------------------------------------------------------------------------- */
typedef struct PdsConvBlockParams {
    const float* weight;
    const float* bias;
    const float* gamma;
    const float* beta;
} PdsConvBlockParams;

/* ------------------------------------------------------------------------------------
 * SubpixelMap.__call__                      reference estimator.py:45-91
 * similarities [batch, planes, height, width] -> disparities [batch, height, width].
 * First-occurrence arg-max, taps j in range(-hw // step, hw // step + 1) (Python floor
 * division), invalid taps get probability 0, result = sum softmax * step * index.
 * ---------------------------------------------------------------------------------- */
int pds_subpixel_map_fwd(const float* similarities, float* disparities,
                         int batch, int planes, int height, int width,
                         int half_support_window, int disparity_step,
                         pds_stream_t stream);

/* SubpixelMap.with_confidence               extends reference estimator.py:45-91 (not in the reference)
 * As pds_subpixel_map_fwd (disparities bit-identical to it), plus confidence [batch, height,
 * width]: the share of the softmax over ALL planes that falls inside the window the disparity
 * uses, c = sum_{k in window} exp(s_k) / sum_k exp(s_k), in (0, 1].  Same single sweep. */
int pds_subpixel_map_confidence_fwd(const float* similarities, float* disparities, float* confidence,
                                    int batch, int planes, int height, int width,
                                    int half_support_window, int disparity_step,
                                    pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Matching.forward, generic-operation path  reference matching.py:12-13, 50-61
 * Builds cat([left, S_d(right)], dim=1) for disparities d_begin .. d_begin+d_count-1:
 * out [d_count, batch, 2*channels, h, w]; S_d(R)[x] = R[x-d] for x >= d else 0.
 * The Python mirror then applies the user's arbitrary `operation` per plane.
 * ---------------------------------------------------------------------------------- */
int pds_shift_concat_fwd(const float* left, const float* right, float* out,
                         int batch, int channels, int h, int w,
                         int d_begin, int d_count, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Matching(maximum_disparity, MatchingOperation()).forward, fused fast path
 *                                           reference matching.py:34-63 + :66-112
 * left/right [batch, features, h, w] -> signatures [batch, sig, d_count, h, w] holding
 * disparities d_begin .. d_begin+d_count-1 (d_begin/d_count shard the disparity axis
 * across GPUs; the whole range is d_begin=0, d_count=maximum_disparity+1).
 * `first` is the bare conv 2*features->features, `blocks` holds 2*residual_blocks
 * conv+LeakyReLU+InstanceNorm2d blocks (ResidualBlock, network_blocks.py:134-144),
 * `last` the bare conv features->sig.  InstanceNorm statistics are per (batch, channel,
 * disparity plane), as in the reference's per-disparity calls.
 * ---------------------------------------------------------------------------------- */
typedef struct PdsMatchingParams {
    int features;            /* 64  */
    int signature_features;  /* 8   */
    int residual_blocks;     /* 2   */
    PdsConvBlockParams first;
    const PdsConvBlockParams* blocks; /* [2 * residual_blocks] */
    PdsConvBlockParams last;
} PdsMatchingParams;

size_t pds_matching_workspace_bytes(const PdsMatchingParams* params, int batch, int h, int w,
                                    int d_count);
int pds_matching_fwd(const PdsMatchingParams* params,
                     const float* left, const float* right, float* signatures,
                     int batch, int h, int w, int d_begin, int d_count,
                     void* workspace, size_t workspace_bytes, int weights_resident,
                     pds_stream_t stream);

/* MatchingOperation.forward on an already concatenated tensor [n, 2*features, h, w]
 * -> [n, sig, h, w]                          reference matching.py:97-112 */
size_t pds_matching_operation_workspace_bytes(const PdsMatchingParams* params, int n, int h, int w);
int pds_matching_operation_fwd(const PdsMatchingParams* params,
                               const float* concatenated, float* signature,
                               int n, int h, int w,
                               void* workspace, size_t workspace_bytes, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Regularization.forward                    reference regularization.py:94-126
 * signatures [batch, F, D, h, w] + left shortcut [batch, F, h, w] -> cost
 * [batch, 2*D, 4*h, 4*w].  D, h, w must be multiples of 16 (four stride-2 levels).
 * ---------------------------------------------------------------------------------- */
typedef struct PdsRegularizationParams {
    int features;                        /* 8 */
    PdsConvBlockParams smoothing;        /* regularization.py:77-78 */
    PdsConvBlockParams contraction[4][2];/* [level][0=_downsampling_2x, 1=_smoothing]  :79-82 */
    PdsConvBlockParams expansion[4][2];  /* [level][0=_upsampling_2x,   1=_smoothing]  :83-86 */
    PdsConvBlockParams upsample_half;    /* :87-89 */
    PdsConvBlockParams upsample_full;    /* bare deconv (3,4,4)/(1,2,2), :90-92 */
} PdsRegularizationParams;

size_t pds_regularization_workspace_bytes(const PdsRegularizationParams* params,
                                          int batch, int d, int h, int w);
int pds_regularization_fwd(const PdsRegularizationParams* params,
                           const float* signatures, const float* left_shortcut, float* cost,
                           int batch, int d, int h, int w,
                           void* workspace, size_t workspace_bytes, int weights_resident,
                           pds_stream_t stream);

/* Eval-mode fusion of Regularization's last layer with SubpixelMap (network.py:50-51):
 * the full-resolution cost volume is never written.  SizeAdapter.unpad (size_adapter.py:45-52)
 * is folded into the store: disparities is the contiguous [batch, 4*h - crop_top,
 * 4*w - crop_left] image without the rows / columns SizeAdapter.pad added on top / left
 * (crop 0, 0: the padded size). */
int pds_regularization_subpixel_map_fwd(const PdsRegularizationParams* params,
                                        const float* signatures, const float* left_shortcut,
                                        float* disparities,
                                        int batch, int d, int h, int w,
                                        int half_support_window, int disparity_step,
                                        int crop_top, int crop_left,
                                        void* workspace, size_t workspace_bytes, int weights_resident,
                                        pds_stream_t stream);

/* Regularization.forward_with_estimator(..., with_confidence=True)   extends network.py:50-51 and
 * estimator.py:45-91 (not in the reference).  As pds_regularization_subpixel_map_fwd (same workspace,
 * same fused / unfused decision, disparities bit-identical to it), plus confidence, stored with the
 * same crop: the window's share of the softmax over all planes (pds_subpixel_map_confidence_fwd). */
int pds_regularization_subpixel_map_confidence_fwd(const PdsRegularizationParams* params,
                                                   const float* signatures, const float* left_shortcut,
                                                   float* disparities, float* confidence,
                                                   int batch, int d, int h, int w,
                                                   int half_support_window, int disparity_step,
                                                   int crop_top, int crop_left,
                                                   void* workspace, size_t workspace_bytes,
                                                   int weights_resident, pds_stream_t stream);

/* Regularization.forward_with_estimator(..., mirror=True)   extends network.py:50-51 (not in the reference).
 * As pds_regularization_subpixel_map_confidence_fwd (same workspace, same fused / unfused decision, confidence
 * nullable), but the cropped columns are stored mirrored: column col of the crop goes to Wc - 1 - col, with
 * Wc = 4w - crop_left, so the result is flip(D, [-1]) of the unmirrored call bit for bit.  The mirror is folded into
 * the fused kernel's store only: where that kernel does not apply the call fails, as a crop does (the caller flips the
 * unfused result itself).  Used for the right-view disparity, flip(forward(flip(R), flip(L))). */
int pds_regularization_subpixel_map_mirrored_fwd(const PdsRegularizationParams* params,
                                                 const float* signatures, const float* left_shortcut,
                                                 float* disparities, float* confidence /* nullable */,
                                                 int batch, int d, int h, int w,
                                                 int half_support_window, int disparity_step,
                                                 int crop_top, int crop_left,
                                                 void* workspace, size_t workspace_bytes,
                                                 int weights_resident, pds_stream_t stream);

/* ContractionBlock3d.forward                reference regularization.py:28-31
 * x [batch, C, D, H, W] -> down, smooth [batch, 2C, D/2, H/2, W/2] (ceil for odd sizes). */
size_t pds_contraction_block_workspace_bytes(int batch, int c, int d, int h, int w);
int pds_contraction_block_fwd(const PdsConvBlockParams* downsampling, const PdsConvBlockParams* smoothing,
                              const float* x, float* down, float* smooth,
                              int batch, int c, int d, int h, int w,
                              void* workspace, size_t workspace_bytes, pds_stream_t stream);

/* ExpansionBlock3d.forward                  reference regularization.py:54-57
 * x [batch, C, D, H, W], shortcut [batch, C/2, 2D, 2H, 2W] -> out like shortcut. */
size_t pds_expansion_block_workspace_bytes(int batch, int c, int d, int h, int w);
int pds_expansion_block_fwd(const PdsConvBlockParams* upsampling, const PdsConvBlockParams* smoothing,
                            const float* x, const float* shortcut, float* out,
                            int batch, int c, int d, int h, int w,
                            void* workspace, size_t workspace_bytes, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * One convolution block of network_blocks.py:47-72 on a plain input tensor x [n, cin, d, h, w]:
 * raw = LeakyReLU(conv(x) + bias) [n, cout, d', h', w'] plus the folded InstanceNorm coefficients
 * (normalised = scale * raw + shift, scale/shift [n*cout] or [n*cout*d'] when per_plane).
 * kd = 1 is Conv2d applied to every d-plane (Matching), kd = 3 is Conv3d; stride 1 or 2.
 * With params->gamma == NULL the block is a bare convolution (scale/shift untouched).
 * This is the launch bench.py times for the roofline of the dominant kernel.
 * ---------------------------------------------------------------------------------- */
size_t pds_conv_block_workspace_bytes(int n, int cin, int cout, int d, int h, int w, int kd, int stride,
                                      int per_plane);
int pds_conv_block_fwd(const PdsConvBlockParams* params, const float* x, float* raw, float* scale,
                       float* shift, int n, int cin, int cout, int d, int h, int w, int kd, int stride,
                       int per_plane, void* workspace, size_t workspace_bytes, pds_stream_t stream);
/* ABI v3 (x_bound: v5).  The same block chained behind another one, as inside the modules (network_blocks.py:47-72:
 * Conv -> LeakyReLU -> InstanceNorm, then the next Conv): x is the producer's RAW output and the loader applies the
 * producer's folded InstanceNorm, x^ = x_scale * x + x_shift ([n*cin], or [n*cin*d] when x_per_plane).  Same workspace
 * size as pds_conv_block_fwd.  This is the form in which the 64 -> 64 layers of MatchingOperation (matching.py:85-88)
 * run in the hot path, and the launch bench.py times for the roofline of the dominant kernel.
 * x_bound: device pointer to ONE float that bounds |x^| (inside the modules in_finalize writes
 * max_c |gamma_c| sqrt(group size) + |beta_c|, which is rigorous), or NULL.  The fp16-split kernels scale their
 * operands by a power of two derived from it, so the bound may be loose by orders of magnitude but must hold; with NULL
 * nothing is assumed about the range and the range-safe forms run (three-way bf16 split / exact fp32). */
int pds_conv_block_chained_fwd(const PdsConvBlockParams* params, const float* x, const float* x_scale,
                               const float* x_shift, int x_per_plane, const float* x_bound, float* raw, float* scale,
                               float* shift, int n, int cin, int cout, int d, int h, int w, int kd, int stride,
                               int per_plane, void* workspace, size_t workspace_bytes, pds_stream_t stream);

/* ABI v7.  One transposed-convolution block of network_blocks.py:37-44 / 75-85 alone, through the dispatch the module
 * walks use (csrc/api.hip deconv_block): x [n, cin, d, h, w] -> raw = LeakyReLU(deconv(x^) + bias).
 * kd = 4: kernel 4 stride 2 padding 1, raw [n, cout, 2d, 2h, 2w]; kd = 3: kernel (3, 4, 4), stride (1, 2, 2), padding 1,
 * raw [n, cout, d, 2h, 2w].  x_scale / x_shift [n*cin]: x is a producer's RAW output behind its folded InstanceNorm,
 * x^ = x_scale * x + x_shift, with x_bound one device float bounding |x^| or NULL (as pds_conv_block_chained_fwd);
 * x_scale == NULL (then x_shift and x_bound are NULL too): x is a plain tensor, x^ = x.  scale / shift [n*cout] receive
 * the folded InstanceNorm of this block; with params->gamma == NULL the block is a bare transposed convolution (no
 * LeakyReLU, no statistics; scale / shift may be NULL).  Tests and measurements of single layers. */
size_t pds_deconv_block_workspace_bytes(int n, int cin, int cout, int d, int h, int w, int kd);
int pds_deconv_block_chained_fwd(const PdsConvBlockParams* params, const float* x, const float* x_scale,
                                 const float* x_shift, const float* x_bound, float* raw, float* scale, float* shift,
                                 int n, int cin, int cout, int d, int h, int w, int kd, void* workspace,
                                 size_t workspace_bytes, pds_stream_t stream);

/* Additive (ABI number unchanged).  One block alone, forward AND backward: a one-layer tape through the reverse walk
 * every pds_*_bwd entry point ends in (csrc/api_training.hip backward_walk), so that a single input gradient can be
 * compared with a reference.  Tests and measurements of single layers.
 *   transposed == 0: convolution, kd 1 | 3, stride 1 | 2 (kd 1: stride 1), per_plane as pds_conv_block_fwd;
 *   transposed != 0: transposed convolution, kd 3 | 4 as pds_deconv_block_chained_fwd (stride is ignored, per_plane 0).
 * x [n, cin, d, h, w] is a plain tensor; x2 (nullable, convolutions only) a second plain tensor of the same shape, the
 * block then runs on x + x2 as the two-source layers of the modules do, and both receive the same input gradient.
 * pds_conv_block_tape_fwd: with params->gamma the raw output, mean and rstd stay in `workspace` -- which the caller keeps
 * untouched until pds_conv_block_bwd, as for every *_bwd below -- and `out` receives the NORMALISED output; with
 * params->gamma == NULL the block is bare (no LeakyReLU, no statistics) and `out` its output.
 * pds_conv_block_bwd: grad_out is the gradient with respect to `out`; grads->weight / bias (/ gamma / beta) and grad_x
 * (and grad_x2, required exactly when x2 is given; it must not alias grad_x) are overwritten.
 * The size queries take norm = (params->gamma != NULL) and two_sources = (x2 != NULL). */
size_t pds_conv_block_tape_workspace_bytes(int transposed, int n, int cin, int cout, int d, int h, int w, int kd,
                                           int stride, int per_plane, int norm, int two_sources);
int pds_conv_block_tape_fwd(const PdsConvBlockParams* params, const float* x, const float* x2, float* out,
                            int transposed, int n, int cin, int cout, int d, int h, int w, int kd, int stride,
                            int per_plane, void* workspace, size_t workspace_bytes, pds_stream_t stream);
size_t pds_conv_block_bwd_workspace_bytes(int transposed, int n, int cin, int cout, int d, int h, int w, int kd,
                                          int stride, int per_plane, int norm, int two_sources);
int pds_conv_block_bwd(const PdsConvBlockParams* params, const PdsConvBlockParams* grads, const float* x,
                       const float* x2, const float* grad_out, float* grad_x, float* grad_x2, int transposed, int n,
                       int cin, int cout, int d, int h, int w, int kd, int stride, int per_plane, void* fwd_workspace,
                       size_t fwd_workspace_bytes, void* workspace, size_t workspace_bytes, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Backward (training: loss.backward() in reference pds_trainer.py:40-46 reaches these modules through
 * autograd).  Each *_bwd re-derives the forward's intermediates from the forward workspace, which the
 * caller must have kept untouched since the matching *_fwd call (the arena layout is deterministic; the
 * library keeps no state).  `grads` mirrors `params`: every pointer is the gradient buffer of that
 * parameter, written (not accumulated).  Input gradients are written too.
 * ---------------------------------------------------------------------------------- */
size_t pds_regularization_bwd_workspace_bytes(const PdsRegularizationParams* params, int batch, int d, int h, int w);
int pds_regularization_bwd(const PdsRegularizationParams* params, const PdsRegularizationParams* grads,
                           const float* signatures, const float* left_shortcut, const float* grad_cost,
                           float* grad_signatures, float* grad_left_shortcut, int batch, int d, int h, int w,
                           void* fwd_workspace, size_t fwd_workspace_bytes, void* workspace, size_t workspace_bytes,
                           pds_stream_t stream);

size_t pds_matching_operation_bwd_workspace_bytes(const PdsMatchingParams* params, int n, int h, int w);
int pds_matching_operation_bwd(const PdsMatchingParams* params, const PdsMatchingParams* grads,
                               const float* concatenated, const float* grad_signature, float* grad_concatenated,
                               int n, int h, int w, void* fwd_workspace, size_t fwd_workspace_bytes,
                               void* workspace, size_t workspace_bytes, pds_stream_t stream);

/* ABI v5.  Matching(MatchingOperation) with gradients (reference matching.py:34-63 under autograd, driven by
 * pds_trainer.py:40-46).  pds_matching_train_fwd is pds_matching_fwd on the differentiable route: layer 0 keeps its
 * factorisation (conv_L(left) + shift_d(conv_R(right)): the [D', B, 128, h, w] concat of matching.py:50-62 never
 * exists), x0 is materialised and every layer output is kept in `workspace`, which the caller preserves until
 * pds_matching_bwd.  pds_matching_bwd walks back from grad_signatures [batch, 8, d_count, h, w] to the parameter
 * gradients (`grads` mirrors `params`, written) and to grad_left / grad_right [batch, features, h, w] (written); layer 0
 * is differentiated through its factorisation: one streaming reduction of d loss / d x0 over the disparity planes, then
 * single-plane convolution gradients.  With d_begin / d_count the gradients are the partial sums of that plane range. */
size_t pds_matching_train_workspace_bytes(const PdsMatchingParams* params, int batch, int h, int w, int d_count);
int pds_matching_train_fwd(const PdsMatchingParams* params, const float* left, const float* right, float* signatures,
                           int batch, int h, int w, int d_begin, int d_count, void* workspace, size_t workspace_bytes,
                           pds_stream_t stream);
size_t pds_matching_bwd_workspace_bytes(const PdsMatchingParams* params, int batch, int h, int w, int d_count);
int pds_matching_bwd(const PdsMatchingParams* params, const PdsMatchingParams* grads, const float* left,
                     const float* right, const float* grad_signatures, float* grad_left, float* grad_right, int batch,
                     int h, int w, int d_begin, int d_count, void* fwd_workspace, size_t fwd_workspace_bytes,
                     void* workspace, size_t workspace_bytes, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Embedding                                 reference embedding.py:11-65 (producer of the path's inputs)
 *   image [batch, input_features, h, w] -> descriptor [batch, features, H4, W4], shortcut [batch, shortcut_features, H4, W4]
 *   H4 = ceil(ceil((h + pad_top) / 2) / 2), W4 likewise.  pad_top / pad_left are the zero rows / columns
 *   SizeAdapter.pad (size_adapter.py:29-43) would have prepended: they are applied virtually, the padded image is
 *   never materialised (the InstanceNorm2d of embedding.py:32 still sees them, as in the reference).
 *   `downsampling` = _embedding_modules.1 / .2 (k5 s2 blocks), `blocks` = 2 * residual_blocks conv blocks of
 *   _embedding_modules.3.., `shortcut` = _shortcut.
 * ---------------------------------------------------------------------------------- */
typedef struct PdsEmbeddingParams {
    int input_features;     /* 3  */
    int features;           /* 64 */
    int shortcut_features;  /* 8  */
    int residual_blocks;    /* 2  */
    PdsConvBlockParams downsampling[2];
    const PdsConvBlockParams* blocks; /* [2 * residual_blocks] */
    PdsConvBlockParams shortcut;
} PdsEmbeddingParams;

size_t pds_embedding_workspace_bytes(const PdsEmbeddingParams* params, int batch, int h, int w, int pad_top,
                                     int pad_left);
int pds_embedding_fwd(const PdsEmbeddingParams* params, const float* image, float* descriptor, float* shortcut,
                      int batch, int h, int w, int pad_top, int pad_left, void* workspace, size_t workspace_bytes,
                      int weights_resident, pds_stream_t stream);
/* Embedding.forward_padded(..., mirror=True)   not in the reference: as pds_embedding_fwd on flip(image, [-1]) (the
 * padding stays on top / left of the MIRRORED image, as SizeAdapter.pad of the flipped image), with the mirror folded
 * into the first layer's loader.  The InstanceNorm statistics are those of the unmirrored image (a mirror does not
 * change them).  Same arguments and workspace (pds_embedding_workspace_bytes) as pds_embedding_fwd; the re-laid-out
 * weights do not depend on the mirror, so weights_resident may carry over between the two.  Inference only. */
int pds_embedding_mirrored_fwd(const PdsEmbeddingParams* params, const float* image, float* descriptor,
                               float* shortcut, int batch, int h, int w, int pad_top, int pad_left, void* workspace,
                               size_t workspace_bytes, int weights_resident, pds_stream_t stream);
/* backward (pds_trainer.py:40-46): needs the untouched forward workspace and the descriptor the forward call
 * returned; grad_descriptor is used as scratch (the shortcut branch's contribution is added to it in place) */
size_t pds_embedding_bwd_workspace_bytes(const PdsEmbeddingParams* params, int batch, int h, int w, int pad_top,
                                         int pad_left);
int pds_embedding_bwd(const PdsEmbeddingParams* params, const PdsEmbeddingParams* grads, const float* image,
                      const float* descriptor, float* grad_descriptor, const float* grad_shortcut, int batch, int h,
                      int w, int pad_top, int pad_left, void* fwd_workspace, size_t fwd_workspace_bytes, void* workspace,
                      size_t workspace_bytes, pds_stream_t stream);
/* ABI v4.  The same backward pass continued to the image (embedding.py:32,46-65 under autograd): grad_image
 * [batch, input_features, h, w] = d loss / d image through the first convolution and the parameter-free
 * InstanceNorm2d of the padded image (the virtual pad pixels take part in its statistics and receive no gradient). */
size_t pds_embedding_image_bwd_workspace_bytes(const PdsEmbeddingParams* params, int batch, int h, int w, int pad_top,
                                               int pad_left);
int pds_embedding_image_bwd(const PdsEmbeddingParams* params, const PdsEmbeddingParams* grads, const float* image,
                            const float* descriptor, float* grad_descriptor, const float* grad_shortcut,
                            float* grad_image, int batch, int h, int w, int pad_top, int pad_left, void* fwd_workspace,
                            size_t fwd_workspace_bytes, void* workspace, size_t workspace_bytes, pds_stream_t stream);

/* backward of the stand-alone blocks (regularization.py:28-31, 54-57 under autograd); grad_* param structs hold
 * the gradient buffers of the two conv blocks, written */
size_t pds_contraction_block_bwd_workspace_bytes(int batch, int c, int d, int h, int w);
int pds_contraction_block_bwd(const PdsConvBlockParams* downsampling, const PdsConvBlockParams* smoothing,
                              const PdsConvBlockParams* grad_downsampling, const PdsConvBlockParams* grad_smoothing,
                              const float* x, const float* grad_down, const float* grad_smooth, float* grad_x,
                              int batch, int c, int d, int h, int w, void* fwd_workspace, size_t fwd_workspace_bytes,
                              void* workspace, size_t workspace_bytes, pds_stream_t stream);
size_t pds_expansion_block_bwd_workspace_bytes(int batch, int c, int d, int h, int w);
int pds_expansion_block_bwd(const PdsConvBlockParams* upsampling, const PdsConvBlockParams* smoothing,
                            const PdsConvBlockParams* grad_upsampling, const PdsConvBlockParams* grad_smoothing,
                            const float* x, const float* shortcut, const float* grad_out, float* grad_x,
                            float* grad_shortcut, int batch, int c, int d, int h, int w, void* fwd_workspace,
                            size_t fwd_workspace_bytes, void* workspace, size_t workspace_bytes, pds_stream_t stream);

/* backward of pds_shift_concat_fwd: grad_out [d_count, batch, 2*channels, h, w] -> grad_left, grad_right
 * [batch, channels, h, w]   (reference matching.py:50-61 under autograd) */
int pds_shift_concat_bwd(const float* grad_out, float* grad_left, float* grad_right, int batch, int channels,
                         int h, int w, int d_begin, int d_count, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * SubpixelCrossEntropy.forward and its gradient      reference loss.py:16-78
 * similarities [n, planes, h, w]; ground_truth [n, h, w] (inf = unknown); weights [n, h, w] or NULL.
 * fwd writes loss[1], lse[n*h*w] (log-sum-exp per pixel, kept for bwd) and stats[2] = {sum w*entropy,
 * denominator}; bwd writes d loss / d similarities scaled by the device scalar grad_loss[1];
 * weights_bwd (ABI v4) writes d loss / d weights [n, h, w] = grad_loss * (entropy - loss) / denominator at known
 * pixels, 0 elsewhere (loss.py:74-77 under autograd; only meaningful when fwd ran with weights).
 * ---------------------------------------------------------------------------------- */
size_t pds_subpixel_cross_entropy_workspace_bytes(int n, int h, int w);
int pds_subpixel_cross_entropy_fwd(const float* similarities, const float* ground_truth, const float* weights,
                                   float* loss, float* lse, float* stats, int n, int planes, int h, int w,
                                   float diversity, int disparity_step, void* workspace, size_t workspace_bytes,
                                   pds_stream_t stream);
int pds_subpixel_cross_entropy_bwd(const float* similarities, const float* ground_truth, const float* weights,
                                   const float* lse, const float* stats, const float* grad_loss,
                                   float* grad_similarities, int n, int planes, int h, int w, float diversity,
                                   int disparity_step, pds_stream_t stream);
int pds_subpixel_cross_entropy_weights_bwd(const float* similarities, const float* ground_truth, const float* lse,
                                           const float* stats, const float* grad_loss, float* grad_weights, int n,
                                           int planes, int h, int w, float diversity, int disparity_step,
                                           pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Evaluation metrics                         reference errors.py:9-74 (pds_trainer.py:48-58)
 *   estimated / ground_truth: `count` floats each (any shape, contiguous); unknown ground truth is +-inf.
 *   pixelwise_absolute_error[count]  = known ? |est - gt| : 0            (may be NULL)
 *   pixelwise_n_pixels_error[count]  = known && |est - gt| > n ? 1 : 0   (may be NULL)
 *   stats[3] (fp64) = { sum of absolute errors over known pixels, known pixels, pixels with error > n }
 *   => mean absolute error = stats[0] / stats[1], n-pixels error [%] = 100 * stats[2] / stats[1] (0 if no pixel known)
 * ---------------------------------------------------------------------------------- */
size_t pds_disparity_errors_workspace_bytes(size_t count);
int pds_disparity_errors_fwd(const float* estimated, const float* ground_truth, size_t count, float n,
                             float* pixelwise_absolute_error, float* pixelwise_n_pixels_error, double* stats,
                             void* workspace, size_t workspace_bytes, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Left-right consistency check                not in the reference
 *   left_disparity / right_disparity: [batch, h, w] (D_L, D_R); the right view's disparity is
 *   D_R(L, R) = flip(forward(flip(R), flip(L)), [-1]).  For a left pixel (b, y, x) with d = D_L[b,y,x]:
 *     k = floorf(((float)x - d) + 0.5f)   (this order of fp32 operations, no multiply)
 *     left_valid[b,y,x] = d finite && 0 <= k < w && fabsf(d - D_R[b,y,k]) <= max_difference
 *   and for the right view, with d = D_R[b,y,x]: k = floorf(((float)x + d) + 0.5f), compared with D_L[b,y,k].
 *   The masks are bytes, 0 or 1.
 *   left_filled / right_filled (nullable, each on its own; must not alias the inputs): the view's disparity with
 *   every invalid pixel replaced by min(D[l], D[r]), l / r the nearest valid pixel to its left / right on the same
 *   row (the one that exists if only one does; a row without a valid pixel is copied unchanged).
 *   max_difference: finite, >= 0.  w < 2^24 (x is exact in fp32).
 * ---------------------------------------------------------------------------------- */
int pds_left_right_check_fwd(const float* left_disparity, const float* right_disparity, unsigned char* left_valid,
                             unsigned char* right_valid, float* left_filled, float* right_filled, int batch, int h,
                             int w, float max_difference, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Rectification and 3-D reprojection             not in the reference
 * Undistortion / rectification of raw frames of a calibrated rig in front of the network and metric points behind it
 * (rectification.py: StereoRig, remap, reproject).  Additive: ABI version unchanged.
 *
 * pds_rectify_maps_fwd: map_x / map_y [h, w] fp32 of one view, as OpenCV initUndistortRectifyMap (CV_32FC1).  Host
 *   double arrays, copied into the kernel arguments: inverse_projection[9] = (P[:3,:3] R_k)^-1 row-major,
 *   camera[5] = fx, fy, cx, cy, skew of the raw camera, distortion[5] = k1, k2, p1, p2, k3.  Per pixel (u, v), in fp64:
 *     (x, y, z) = iP (u, v, 1); x /= z; y /= z; r2 = x^2 + y^2; kr = 1 + ((k3 r2 + k2) r2 + k1) r2
 *     xd = x kr + 2 p1 x y + p2 (r2 + 2 x^2);  yd = y kr + p1 (r2 + 2 y^2) + 2 p2 x y
 *     map_x = fx xd + skew yd + cx;  map_y = fy yd + cy      (each rounded once to fp32)
 *
 * pds_remap_fwd: out [batch, 3, h_out, w_out] fp32 = bilinear sample of image at (map_x, map_y) [h_out, w_out].
 *   layout 0: image float32 [batch, 3, h_in, w_in]; layout 1: image uint8 [batch, h_in, w_in, 3] (values are not
 *   rescaled: 200 -> 200.0f).  x0 = floorf(mx), ax = mx - x0 (same in y); out = (1-ay)((1-ax) p00 + ax p01) +
 *   ay((1-ax) p10 + ax p11); a tap outside the image reads border_value (finite), a non-finite map entry gives
 *   border_value.  Integer maps reproduce the source bit for bit.  reverse_channels != 0: output channel c reads input
 *   channel 2 - c (BGR -> RGB).  batch * 3 * h * w < 2^31 on both sides, h_in, w_in < 2^24.
 *
 * pds_reproject_fwd: (X, Y, Z, W) = M (x, y, d, 1) in fp32, M = matrix[16] (host, row-major, copied into the kernel
 *   arguments), x / y the column / row of disparity [batch, h, w], d its value.  points [batch, h, w, 3] = (X, Y, Z) / W,
 *   depth [batch, h, w] = Z / W; either may be null, not both.  NaN in every output where d is not finite or d <= 0,
 *   W <= 0 (or NaN), valid (torch.bool [batch, h, w], nullable) is 0, or confidence (nullable) is not >= min_confidence.
 *   batch * h * w * 3 < 2^31.
 * ---------------------------------------------------------------------------------- */
int pds_rectify_maps_fwd(const double* inverse_projection, const double* camera, const double* distortion,
                         float* map_x, float* map_y, int h, int w, pds_stream_t stream);
int pds_remap_fwd(const void* image, int layout, const float* map_x, const float* map_y, float* out, int batch,
                  int h_in, int w_in, int h_out, int w_out, float border_value, int reverse_channels,
                  pds_stream_t stream);
int pds_reproject_fwd(const float* disparity, const unsigned char* valid, const float* confidence,
                      float min_confidence, const float* matrix, float* points, float* depth, int batch, int h, int w,
                      pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Speckle filter: regions of similar disparity by connected components         not in the reference
 * Additive: ABI version unchanged.  For every image [h, w] of disparity [batch, h, w] on its own:
 *   eligible(p)  = D[p] finite && (valid == NULL || valid[p] != 0)          (valid: bytes, torch.bool or uint8)
 *   linked(p, q) = p, q eligible horizontal or vertical neighbours && fabsf(D[p] - D[q]) <= max_difference
 *                  (one fp32 subtraction; links are per neighbour pair, as OpenCV filterSpeckles: a smooth ramp is one
 *                  region although its ends differ by far more than max_difference)
 *   region       = connected component of eligible pixels under these links (4-connectivity)
 *   sizes[p]     = pixels of p's region, 0 where p is not eligible                             (int32, nullable)
 *   keep[p]      = eligible(p) && sizes[p] > max_size      (bytes 0 / 1; a region of exactly max_size pixels is removed,
 *                  max_size = 0 keeps every eligible pixel)
 *   filtered[p]  = keep[p] ? D[p] : fill_value             (nullable; fill_value any float, NaN included)
 * Exact and reproducible: integer atomics only, and the outputs do not depend on the order in which they land.
 * filtered may BE disparity (in place: a pixel is read and written by the same thread of the last pass); any other
 * overlap between an output and an input or another output is refused.
 * max_difference finite and >= 0, max_size >= 0, h * w <= 2^31 - 1 (32-bit labels), batch * h * w <= 2^31 - 1 - 2^22.
 * workspace: pds_speckle_filter_workspace_bytes(batch, h, w) bytes (8 per pixel + 256; 0 and an error message for a
 * shape the entry point refuses), contents undefined before and after.  Four launches at most on `stream`, their number
 * a function of the shape alone; no host synchronisation, no copy.
 * ---------------------------------------------------------------------------------- */
size_t pds_speckle_filter_workspace_bytes(int batch, int h, int w);
int pds_speckle_filter_fwd(const float* disparity, const unsigned char* valid, unsigned char* keep, float* filtered,
                           int* sizes, int batch, int h, int w, float max_difference, int max_size, float fill_value,
                           void* workspace, size_t workspace_bytes, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Hole-aware median filter of a disparity map                                    not in the reference
 * Additive: ABI version unchanged.  The stage after the speckle filter (OpenCV: filterSpeckles, then medianBlur), but
 * aware of NaN and masks.  For every image [h, w] of disparity [batch, h, w] on its own:
 *   k            = kernel_size, one of 3, 5, 7;  r = k / 2
 *   eligible(q)  = D[q] finite && (valid == NULL || valid[q] != 0)          (the speckle filter's rule)
 *   W(p)         = { q : |qx - px| <= r, |qy - py| <= r, q inside the image, eligible(q) }
 *                  (the window is CLIPPED at the border: nothing is replicated or mirrored)
 *   n(p)         = |W(p)|                                                      0 .. k*k
 *   median(p)    = the value of rank (n - 1) / 2 (0-based, ascending) among D[W(p)]:  the LOWER median.
 *                  No two samples are ever averaged, so the output never invents a disparity between a
 *                  foreground and a background surface, and for even n the farther surface wins, as in the
 *                  left-right check's fill.
 *   out[p], ok[p] =  median(p), 1      if eligible(p)                                   (n >= 1: p is in W)
 *                    median(p), 1      if not eligible(p) and fill_holes and n(p) >= min_valid
 *                    fill_value, 0     otherwise
 *   min_valid    in 1 .. k*k (the Python mirror's default: k*k / 2 + 1, a majority of the full window)
 * filtered may not overlap disparity, and ok (bytes 0 / 1, nullable) may not overlap valid (neighbours are read); any
 * other overlap of an output with an input or the other output is refused as well.  -0.0 and +0.0 compare equal, and
 * either may be returned when both are in the window; apart from that the output is one of the window's inputs bit for
 * bit (denormals included: the selection compares integer keys).  fill_value is written as given (any float, NaN
 * included).  Exact and reproducible.  batch * h * w <= 2^31 - 1.  No workspace; one launch on `stream`, no atomics, no
 * host synchronisation, no copy.
 * ---------------------------------------------------------------------------------- */
int pds_median_filter_fwd(const float* disparity, const unsigned char* valid /* or NULL */,
                          float* filtered, unsigned char* ok /* or NULL */,
                          int batch, int h, int w, int kernel_size, int fill_holes, int min_valid,
                          float fill_value, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Packed, coloured point cloud: ordered compaction of the reprojection            not in the reference
 * Additive: ABI version unchanged.  The last stage: what pds_reproject_fwd would write as points [batch, h, w, 3],
 * without the rejected pixels.  For pixel p of batch entry b (disparity, valid, confidence, min_confidence, matrix as
 * pds_reproject_fwd):
 *   keep(p)      = pds_reproject_fwd's point at p is not NaN:  d finite && d > 0 && W > 0 && (valid == NULL ||
 *                  valid[p] != 0) && (confidence == NULL || confidence[p] >= min_confidence)   (a NaN confidence fails;
 *                  evaluated as "x of that point is not NaN", what ~isnan(points[..., 0]) keeps of the dense output)
 *                  && min_depth <= Z/W <= max_depth, on the fp32 quotient itself: a pixel whose depth EQUALS a bound is
 *                  kept.  min_depth = -inf / max_depth = +inf: no bound.
 *   order        = raster order within an entry, entries in batch order
 *   points       [N, 3] fp32: the kept points, bit-identical to what pds_reproject_fwd writes at that pixel (one device
 *                function serves both entry points)
 *   colors       [N, 3], nullable: the pixel of `image` (nullable; the rectified left image) at the same position,
 *                copied, not rescaled.  image_layout 0: image float32 [batch, 3, h, w] -> colors float32;
 *                image_layout 1: image uint8 [batch, h, w, 3] -> colors uint8   (pds_remap_fwd's two layouts)
 *   index        [N] int32, nullable: y * w + x of the pixel within its entry
 *   offsets      [batch + 1] int32: entry b owns rows [offsets[b], offsets[b + 1]); offsets[batch] is the TRUE number of
 *                kept pixels even when it exceeds capacity
 *   capacity     rows the output buffers hold (>= 0): only the first `capacity` points in order are written and nothing
 *                is written past them; offsets[batch] > capacity tells the caller that the cloud was cut
 * Exact and reproducible: integer arithmetic only in the ordering, no floating-point atomics, the same bits on every
 * run.  Three launches on `stream` (count per tile of 1024 pixels, scan of the tile counts, scatter); no workgroup waits
 * on another, no host synchronisation, no copy.  No output may overlap an input or another output.
 * batch * h * w <= 2^31 - 1.  workspace: pds_point_cloud_workspace_bytes(batch, h, w) bytes (4 per tile + 256; 0 and an
 * error message for a shape the entry point refuses), contents undefined before and after.
 * ---------------------------------------------------------------------------------- */
size_t pds_point_cloud_workspace_bytes(int batch, int h, int w);
int pds_point_cloud_fwd(const float* disparity, const unsigned char* valid /* or NULL */,
                        const float* confidence /* or NULL */, float min_confidence, const float* matrix /* [16] */,
                        float min_depth, float max_depth,
                        const void* image /* or NULL */, int image_layout /* 0: f32 NCHW, 1: u8 NHWC */,
                        float* points, void* colors /* or NULL */, int* index /* or NULL */, int* offsets,
                        long long capacity, int batch, int h, int w,
                        void* workspace, size_t workspace_bytes, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Depth registration: z-buffered forward warp into another camera                  not in the reference
 * Additive: ABI version unchanged.  Everything behind the network lives on the pixel grid of the rectified left view;
 * this carries the depth onto the grid of another camera (the raw left frame, the right view, a colour camera), as
 * OpenCV rgbd::registerDepth, ROS depth_image_proc/register, RealSense align.  disparity, valid, confidence,
 * min_confidence as pds_reproject_fwd.  matrix[16] = M' = [[R, t], [0, 0, 0, 1]] * M (host, row-major, composed in fp64
 * and rounded once; M the matrix pds_reproject_fwd takes, [R | t] the pose of the target camera in M's frame): source
 * pixel + disparity -> point in the TARGET camera frame.  camera[5] = fx, fy, cx, cy, skew
 * and distortion[5] = k1, k2, p1, p2, k3 of the target camera (the model of pds_rectify_maps_fwd), target [ht, wt].
 * Per source pixel p (raster index y * w + x within its batch entry), in fp32:
 *   1. (X, Y, Z) = pds_reproject_fwd's point at p for M' (one device function serves both entry points): kept iff d
 *      finite && d > 0 && W > 0 && (valid == NULL || valid[p] != 0) && (confidence == NULL || confidence[p] >=
 *      min_confidence).  Dropped unless Z is finite and Z > 0.
 *   2. x = X / Z, y = Y / Z, r2 = x^2 + y^2.  Dropped when 1 + 3 k1 r2 + 5 k2 r2^2 + 7 k3 r2^3 <= 0: there the radial
 *      model has folded back, and a point far outside the field of view would otherwise land inside the image.  (OpenCV's
 *      projectPoints has no such guard.)
 *   3. kr = 1 + ((k3 r2 + k2) r2 + k1) r2;  xd = x kr + 2 p1 x y + p2 (r2 + 2 x^2);  yd = y kr + p1 (r2 + 2 y^2) + 2 p2 x y
 *      u = fx xd + skew yd + cx;  v = fy yd + cy.  Dropped if u or v is not finite.
 *   4. footprint: splat 1: the one pixel (floorf(u + 0.5f), floorf(v + 0.5f)); splat 2: the four pixels {floorf(u),
 *      floorf(u) + 1} x {floorf(v), floorf(v) + 1}, which closes the one-pixel cracks a forward warp leaves when the
 *      target samples the surface more densely than the source.  Footprint pixels outside [0, wt) x [0, ht) are skipped
 *      one by one.
 *   5. every footprint pixel receives key = (uint64(float_as_uint(Z)) << 32) | uint32(p) by a 64-bit unsigned atomic
 *      minimum (Z > 0 and finite: its bits order as its value).
 * Then every target pixel t is resolved:
 *   never written:  depth[t] = fill_value (any float, NaN included), index[t] = -1, valid_out[t] = 0
 *   written:        depth[t] = the winning Z, bit for bit, index[t] = the winning p, valid_out[t] = 1
 * depth [batch, ht, wt] fp32; index [batch, ht, wt] int32, nullable; valid_out [batch, ht, wt] bytes 0 / 1, nullable.
 * The nearest point wins, among equal depths the smaller source index.  The minimum of integers does not depend on
 * arrival order: the same bits on every run and on every stream; no floating-point atomic is involved.
 * Limit: with a target much denser than the source, background can show through foreground even with splat 2; there is
 * no hole filling (pds_median_filter_fwd with fill_holes on the registered depth is the tool for that).
 * splat 1 or 2; matrix, camera, distortion and min_confidence finite; h * w, ht * wt, batch * h * w and batch * ht * wt
 * <= 2^31 - 1.  No output may overlap an input or another output.  workspace: pds_register_depth_workspace_bytes(batch,
 * ht, wt) bytes (the key buffer: 8 per target pixel, rounded up to 256; 0 and an error message for a shape the entry point
 * refuses), 8-byte aligned, contents undefined before and after.  On `stream`: the key buffer is cleared
 * (hipMemsetAsync), then two launches (scatter over source pixels, resolve over target pixels); no workgroup waits on
 * another, no host synchronisation, no copy.
 * ---------------------------------------------------------------------------------- */
size_t pds_register_depth_workspace_bytes(int batch, int ht, int wt);
int pds_register_depth_fwd(const float* disparity, const unsigned char* valid /* or NULL */,
                           const float* confidence /* or NULL */, float min_confidence,
                           const float* matrix /* [16] */, const float* camera /* [5] */,
                           const float* distortion /* [5] */, int splat, float fill_value,
                           float* depth, int* index /* or NULL */, unsigned char* valid_out /* or NULL */,
                           int batch, int h, int w, int ht, int wt,
                           void* workspace, size_t workspace_bytes, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Surface normals from disparity: edge-aware plane fit                             not in the reference
 * Additive: ABI version unchanged.  How the surface at a pixel is oriented, for a mesher, point-to-plane ICP, a viewer that
 * shades, Poisson reconstruction.  Stereo noise is uniform in disparity, not in depth, and a projective map takes planes
 * to planes: a plane is fitted to d(x, y) over a small window, and its image under the matrix is a 3-D plane whose normal
 * is the answer.  disparity, valid, confidence, min_confidence, matrix as pds_reproject_fwd (matrix[16] = M, host,
 * row-major, rounded once to fp32).  For every image [h, w] of disparity [batch, h, w] on its own and every pixel
 * p = (x0, y0) with d0 = D[p]:
 *   k            = kernel_size, one of 3, 5, 7;  r = k / 2
 *   kept(p)      = pds_reproject_fwd keeps p (one device function serves both entry points): d0 finite && d0 > 0 &&
 *                  W > 0 && (valid == NULL || valid[p] != 0) && (confidence == NULL || confidence[p] >= min_confidence)
 *   eligible(q)  = D[q] finite && D[q] > 0 && (valid == NULL || valid[q] != 0) && (confidence == NULL ||
 *                  confidence[q] >= min_confidence)                                     (a NaN confidence fails)
 *   delta(q)     = D[q] - d0                                                            (ONE fp32 subtraction)
 *   W(p)         = { q : |qx - x0| <= r, |qy - y0| <= r, q inside the image, eligible(q), fabsf(delta(q)) <=
 *                  max_difference }     (the window is CLIPPED at the border: nothing is replicated or mirrored; the
 *                  test on delta keeps the fit on p's side of a depth edge; max_difference = +inf: no such test)
 *   i, j         = qx - x0, qy - y0                                                     (integers)
 *   n, Si, Sj, Sii, Sij, Sjj = the sums of 1, i, j, i i, i j, j j over W(p)             (integers)
 *   A = n Sii - Si^2, Bm = n Sij - Si Sj, C = n Sjj - Sj^2, det = A C - Bm^2            (exact integers, 32 bits suffice)
 *   degenerate(p) = !kept(p) || n < min_valid || det == 0      (det == 0 <=> the pixels of W(p) are collinear: decided
 *                  in integers)
 *   Sd, Sid, Sjd = the fp32 sums of delta, i delta, j delta over W(p)
 *   u = n Sid - Si Sd,  v = n Sjd - Sj Sd
 *   a = (C u - Bm v) / det,  b = (A v - Bm u) / det,  c0 = (Sd - a Si - b Sj) / n
 *                  (the least-squares plane delta = a i + b j + c0)
 *   dh = d0 + c0;  H = M (x0, y0, dh, 1)^T;  X = H[:3] / H[3]      (degenerate too if H[3] <= 0 or not finite)
 *   t_x = (M[:3,0] - X M[3,0]) + a (M[:3,2] - X M[3,2])
 *   t_y = (M[:3,1] - X M[3,1]) + b (M[:3,2] - X M[3,2])
 *                  (the Jacobian of the homogeneous division along x and along y, its common 1 / H[3] dropped)
 *   N = t_x x t_y;  degenerate if |N|^2 is 0 or not finite;  N /= |N|;  N = -N if N . (X - viewpoint) > 0
 *                  (a component that is -0 is written as +0)
 *   normals[p]   = degenerate(p) ? (fill_value, fill_value, fill_value) : N      [batch, h, w, 3] fp32: a unit vector that
 *                  faces the viewpoint; fill_value is written as given (any float, NaN included)
 *   valid_out[p] = !degenerate(p)                                               [batch, h, w] bytes 0 / 1, nullable
 *   min_valid    in 3 .. k*k (the Python mirror's default: k*k / 2 + 1, a majority of the full window)
 *   viewpoint    [3] (host), NULL = the origin of the matrix's frame
 * Membership of W(p), n and the degeneracy test are exact (one fp32 subtraction, then integers); no atomic is involved,
 * so the output has the same bits on every run and on every stream.  kernel_size 3, 5 or 7; max_difference >= 0 (+inf
 * allowed, NaN refused); min_confidence, matrix and viewpoint finite; the float pointers 4-byte aligned;
 * batch * h * w <= 2^31 - 1; no output may overlap an input or the other output.  No workspace; one launch on `stream`
 * (a tile of 64 x 16 pixels plus its halo staged in LDS once, the 12-byte records leaving through LDS as 16-byte stores
 * wherever the address allows), no host synchronisation, no copy.
 * ---------------------------------------------------------------------------------- */
int pds_surface_normals_fwd(const float* disparity, const unsigned char* valid /* or NULL */,
                            const float* confidence /* or NULL */, float min_confidence,
                            const float* matrix /* host, [16] */, const float* viewpoint /* host, [3], NULL = origin */,
                            int kernel_size, float max_difference, int min_valid, float fill_value,
                            float* normals, unsigned char* valid_out /* or NULL */,
                            int batch, int h, int w, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Triangle mesh from disparity: edge-aware faces over the packed cloud            not in the reference
 * Additive: ABI version unchanged.  A disparity map is a regular grid: the mesh is two triangles per 2 x 2 cell of
 * pixels, cut wherever a depth edge runs through the cell.  A mesh is a cloud plus faces.
 *   inputs       disparity, valid, confidence, min_confidence, matrix, min_depth, max_depth, image, image_layout exactly
 *                as pds_point_cloud_fwd; max_difference >= 0 (+inf allowed, NaN and negative values refused); flip 0 / 1
 *   vertices     points, colors, index, offsets, capacity: what pds_point_cloud_fwd writes for the same arguments, bit
 *                for bit and in the same order (the same kernels, the same keep predicate, the same reprojection of one
 *                pixel).  A kept pixel that ends up in no face stays a vertex.
 *   edges        two kept pixels p, q of one entry are joined iff fabsf(D[p] - D[q]) <= max_difference: ONE fp32
 *                subtraction of the input disparities (the rule of pds_surface_normals_fwd)
 *   cells        for x in [0, w - 2] and y in [0, h - 2] of entry b the corners  a = (x, y)      b = (x + 1, y)
 *                                                                                 c = (x, y + 1)  e = (x + 1, y + 1)
 *                (no cell at x = w - 1: none spans two rows' ends; none at y = h - 1: none spans two entries).  A
 *                triangle is emitted iff its three corners are kept and its three edges are joined, the diagonal included.
 *                  four corners kept:   the diagonal is a-e iff fabsf(D[a] - D[e]) < fabsf(D[b] - D[c]); otherwise, ties
 *                                       included, it is b-c.  Diagonal b-c: the candidates (a, c, b) then (b, c, e);
 *                                       diagonal a-e: (a, c, e) then (a, e, b).  No fallback to the other diagonal (its
 *                                       difference is at least as large).
 *                  three corners kept:  the one candidate of the lists above that avoids the missing corner:
 *                                       e missing: (a, c, b)   a missing: (b, c, e)   b missing: (a, c, e)
 *                                       c missing: (a, e, b)
 *                  fewer:               nothing
 *   winding      the vertex order is as listed; flip != 0 swaps the second and the third vertex of every face.  The
 *                listed order faces a camera at the origin, ((p1 - p0) x (p2 - p0)) . p0 < 0, for a matrix with X right,
 *                Y down, Z forward.
 *   order        faces are ordered by the flat index of their corner a (raster order within an entry, entries in batch
 *                order); within a cell the first candidate comes before the second
 *   faces        [F, 3] int32: rows of `points`, counted over the whole batch (entry b's own numbering: subtract
 *                offsets[b]).  With capacity smaller than the number of kept pixels the faces still hold the true rows;
 *                offsets[batch] > capacity tells the caller that the vertices were cut.
 *   face_offsets [batch + 1] int32: entry b owns faces [face_offsets[b], face_offsets[b + 1]); face_offsets[batch] is the
 *                TRUE number of faces even when it exceeds face_capacity
 *   face_capacity  rows `faces` holds (>= 0): only the first face_capacity faces in order are written and nothing is
 *                written past them
 * Exact and reproducible: every output is an integer or a bit-copy, integer arithmetic only in the ordering, no
 * floating-point atomics, the same bits on every run and on every stream.  Six launches on `stream`: the three of
 * pds_point_cloud_fwd, whose scatter also writes a dense int32 rank map (the packed row of each pixel, -1 where it is not
 * kept) into the workspace; the face count per tile of 1024 anchor pixels; the scan of those counts; the face scatter.
 * No workgroup waits on another, no host synchronisation, no copy.  No output may overlap an input or another output.
 * 2 * batch * h * w <= 2^31 - 1 (a face per half cell must be countable in 32 bits).  workspace:
 * pds_triangle_mesh_workspace_bytes(batch, h, w) bytes (twice pds_point_cloud_workspace_bytes + 4 per pixel rounded up to
 * 256; 0 and an error message for a shape the entry point refuses), 16-byte aligned, contents undefined before and after.
 * ---------------------------------------------------------------------------------- */
size_t pds_triangle_mesh_workspace_bytes(int batch, int h, int w);
int pds_triangle_mesh_fwd(const float* disparity, const unsigned char* valid /* or NULL */,
                          const float* confidence /* or NULL */, float min_confidence, const float* matrix /* [16] */,
                          float min_depth, float max_depth, float max_difference, int flip,
                          const void* image /* or NULL */, int image_layout /* 0: f32 NCHW, 1: u8 NHWC */,
                          float* points, void* colors /* or NULL */, int* index /* or NULL */, int* offsets,
                          long long capacity, int* faces, int* face_offsets, long long face_capacity,
                          int batch, int h, int w,
                          void* workspace, size_t workspace_bytes, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * TSDF fusion: integrate disparity maps into a volume, extract its surface         not in the reference
 * Additive: ABI version unchanged.  Stereo depth noise grows with Z^2; frames of a moving rig are fused into one dense,
 * bounded truncated-signed-distance volume (KinectFusion, Open3D TSDFVolume.integrate / extract_point_cloud).
 * The volume is the caller's: tsdf and weight, fp32 [nz, ny, nx], x fastest, voxel v = (k * ny + j) * nx + i; a fresh
 * volume holds tsdf = 1, weight = 0.
 *
 * pds_tsdf_integrate_fwd.  disparity, valid, confidence, min_confidence, matrix as pds_reproject_fwd ([batch, h, w];
 * matrix[16] rounded once to fp32).  transforms [batch][12] (host): per entry A (3 x 3, row-major) then b (3), the map
 * from voxel indices to the frame the matrix produces, p_c = A (i, j, k) + b (the Python mirror: A = voxel_size R,
 * b = R (origin + voxel_size / 2) + t for the pose [R | t] from the world into that frame; fp64, rounded once).
 * camera[5] = fx, fy, cx, cy, skew: the pinhole of that frame.  The entries are integrated one after the other, b = 0 ..
 * batch - 1, two launches each:
 *   tsdf_depth      per source pixel p: Z = the z of pds_reproject_fwd's point at p (one device function serves both):
 *                   kept iff d finite && d > 0 && W > 0 && (valid == NULL || valid[p] != 0) && (confidence == NULL ||
 *                   confidence[p] >= min_confidence); the workspace receives Z, or NaN where the pixel is dropped or Z is
 *                   not finite and positive, and beside it confidence[p] iff weight_by_confidence != 0
 *   tsdf_integrate  per voxel (i, j, k), in fp32:
 *     1. p_c = A (i, j, k) + b; skipped unless z_c > 0
 *     2. x = x_c / z_c, y = y_c / z_c, u = fx x + skew y + cx, v = fy y + cy; skipped unless both are finite
 *     3. px = floorf(u + 0.5f), py = floorf(v + 0.5f)                      (the rounding of pds_register_depth_fwd, splat 1)
 *     4. skipped outside [0, w) x [0, h) or where the stored Z is NaN
 *     5. sdf = Z - z_c; skipped where sdf < -truncation
 *     6. t = min(1, sdf / truncation)
 *     7. wt = 1, or with weight_by_confidence the pixel's confidence; skipped unless wt > 0
 *     8. tsdf[v] = (tsdf[v] * weight[v] + t * wt) / (weight[v] + wt)
 *     9. weight[v] = min(weight[v] + wt, max_weight)
 * A skipped voxel is neither read nor written, and whether a voxel is skipped does not depend on its old state: the
 * traffic is that of the updated share of the volume.  Each voxel belongs to one thread: no atomics, the same bits on every
 * run and on every stream, whatever the alignment of tsdf and weight (4 bytes suffice; where both share one misalignment
 * against 16 bytes, runs of four updated voxels are loaded and stored as 16 bytes).  truncation > 0 and finite;
 * max_weight > 0; min_confidence, matrix, transforms, camera finite; weight_by_confidence needs a confidence;
 * nx, ny, nz <= 2^24 each (a voxel index is an exact float); 3 * nx * ny * nz, h * w and batch * h * w <= 2^31 - 1.  tsdf, weight and the workspace may not overlap one another or an
 * input.  workspace: pds_tsdf_integrate_workspace_bytes(h, w) bytes (two planes of 4 bytes per pixel, each rounded up to
 * 256: Z and the weights of ONE entry, reused by the next in stream order; 0 and an error message for a shape the entry
 * point refuses), 16-byte aligned, contents undefined before and after.  No workgroup waits on another, no host
 * synchronisation, no copy.
 *
 * pds_tsdf_extract_fwd.  A voxel is observed iff weight[v] >= min_weight.  For every voxel v = (i, j, k) and axis
 * a = 0, 1, 2 (+x, +y, +z) with n the neighbour of v along a: if n lies inside the volume, both are observed and
 * (tsdf[v] < 0) != (tsdf[n] < 0), the edge holds a surface point:
 *   r        = tsdf[v] / (tsdf[v] - tsdf[n])                                                        (fp32)
 *   point    = origin + voxel_size * ((i, j, k) + 0.5 + r e_a)
 *   index    = 3 v + a; the points come in ascending index
 *   normal   = normalise((1 - r) g(v) + r g(n)) with the central differences g(c)_m = tsdf[c + e_m] - tsdf[c - e_m]; the
 *              tsdf is positive towards the camera, so the normal faces the viewer.  (NaN, NaN, NaN) where one of the twelve
 *              stencil voxels is outside the volume or unobserved or where the interpolated gradient is zero; the point stays.
 * points [capacity, 3] fp32; normals [capacity, 3] fp32, nullable; index [capacity] int32, nullable; offsets [2] int32:
 * offsets[0] = 0, offsets[1] = the TRUE number of surface points even when it exceeds capacity (>= 0): only the first
 * `capacity` points in order are written and nothing is written past them.  origin[3] (host) finite, voxel_size > 0 and
 * finite, min_weight not NaN.  The decisions (observed, sign, order) are exact on the stored bits: the same count and the
 * same index on every run and on every stream.  Three launches in the pattern of pds_point_cloud_fwd (tsdf_extract_count
 * per tile of 1024 voxels, tsdf_extract_scan, tsdf_extract_scatter with LDS-staged contiguous stores); no workgroup waits
 * on another, no host synchronisation, no copy.  No output may overlap an input or another output.  workspace:
 * pds_tsdf_extract_workspace_bytes(nx, ny, nz) bytes (4 per tile of 1024 voxels rounded up to 256, plus 256; 0 and an
 * error message for a volume the entry point refuses), 4-byte aligned, contents undefined before and after.
 * ---------------------------------------------------------------------------------- */
size_t pds_tsdf_integrate_workspace_bytes(int h, int w);
int pds_tsdf_integrate_fwd(const float* disparity, const unsigned char* valid /* or NULL */,
                           const float* confidence /* or NULL */, float min_confidence, int weight_by_confidence,
                           const float* matrix /* host, [16] */, const float* transforms /* host, [batch][12] */,
                           const float* camera /* host, [5] */, float truncation, float max_weight,
                           float* tsdf, float* weight, int nx, int ny, int nz, int batch, int h, int w,
                           void* workspace, size_t workspace_bytes, pds_stream_t stream);
size_t pds_tsdf_extract_workspace_bytes(int nx, int ny, int nz);
int pds_tsdf_extract_fwd(const float* tsdf, const float* weight, const float* origin /* host, [3] */,
                         float voxel_size, float min_weight, float* points, float* normals /* or NULL */,
                         int* index /* or NULL */, int* offsets /* [2] */, long long capacity,
                         int nx, int ny, int nz, void* workspace, size_t workspace_bytes, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * TSDF mesh: the volume's surface as a closed triangle mesh (marching tetrahedra)    not in the reference
 * Additive: ABI version unchanged.  The fused model as a surface: the crossings of pds_tsdf_extract_fwd along seven edge
 * directions instead of three, joined into faces by marching tetrahedra on the Kuhn triangulation of each cell (six
 * tetrahedra around the body diagonal).  Sixteen sign cases per tetrahedron, no 256-case table; neighbouring cells agree
 * on the diagonal of every shared face, so the mesh is closed wherever the volume is observed.  The volume, `observed`
 * (weight[v] >= min_weight) and v = (k * ny + j) * nx + i are those of pds_tsdf_extract_fwd.
 *   edges      a direction d = 1 .. 7 is a bit mask with offset(d) = (d & 1, (d >> 1) & 1, (d >> 2) & 1): 1, 2, 4 the axes,
 *              3, 5, 6 the face diagonals, 7 the body diagonal.  The edge (v, d) joins voxel v to n = v + offset(d) where n
 *              lies inside the volume.
 *   vertices   an edge carries a vertex iff both ends are observed and (tsdf[v] < 0) != (tsdf[n] < 0):
 *                r      = tsdf[v] / (tsdf[v] - tsdf[n])                                                 (fp32)
 *                point  = origin + voxel_size * ((i, j, k) + 0.5 + r offset(d))
 *                index  = 7 v + (d - 1); the vertices come in ascending index
 *                normal = normalise((1 - r) g(v) + r g(n)), g and the NaN rule as pds_tsdf_extract_fwd
 *              For d = 1, 2, 4 point and normal are those of pds_tsdf_extract_fwd for a = 0, 1, 2, bit for bit (one device
 *              function serves both).  A vertex is emitted whether or not a face uses it: on the rim of the observed region
 *              vertices may be unreferenced.
 *   cells      cell c is the cell whose corner 0 is voxel c, for i < nx - 1, j < ny - 1, k < nz - 1; corner m = 0 .. 7
 *              sits at offset(m).  Tetrahedron t = 0 .. 5 belongs to the axis permutation (a, b, e) in lexicographic
 *              order, (0,1,2) (0,2,1) (1,0,2) (1,2,0) (2,0,1) (2,1,0): its corners are p0 = 0, p1 = 1 << a,
 *              p2 = p1 | 1 << b, p3 = 7.  Its edge (pm, pn), m < n, is the edge (voxel of pm, d = pn ^ pm) above.
 *   faces      a tetrahedron emits faces iff its four corners are observed.  With s_m = (tsdf < 0) at p_m:
 *                one corner A alone on its side (the others B < C < D by position): the triangle (AB, AC, AD)
 *                two against two (the negative pair A < B, the others C < D, by position): (AC, AD, BD) then (AC, BD, BC)
 *                all alike: nothing
 *              winding: by the right-hand rule the face normal points from the negative corners towards the positive
 *              ones -- towards the viewer, like the normals; where the listed order does not, its second and third vertex
 *              are swapped.  That is decided as if every vertex sat at the midpoint of its edge: a function of
 *              (t, s_0 .. s_3) alone, a table of 6 x 16 bits, never a floating-point test on the points.
 *              Faces are ordered by 6 c + t, within a tetrahedron as listed.  faces [face_capacity, 3] int32: rows of
 *              `points`; with `capacity` below the number of vertices they still hold the true rows.
 * points [capacity, 3] fp32; normals [capacity, 3] fp32, nullable; index [capacity] int32, nullable; offsets [2] and
 * face_offsets [2] int32: [0] = 0, [1] = the TRUE number of vertices / faces even beyond the capacities (>= 0): only the
 * first `capacity` vertices and `face_capacity` faces in order are written and nothing is written past them.  A volume
 * without cells (a dimension of 1) has vertices and no faces.  Every decision (observed, sign, case, winding, order) is
 * exact on the stored bits.  Six launches on `stream`: tsdf_mesh_count per tile of 1024 voxels, tsdf_mesh_scan,
 * tsdf_mesh_scatter (LDS-staged contiguous stores; it also writes per voxel the row of its first vertex and its mask of
 * seven edge bits into the workspace, so that the vertex of edge (v, d) is row first[v] + popcount(mask[v] & ((1 << (d - 1))
 * - 1)), without a search), tsdf_mesh_face_count per tile of 1024 cells, tsdf_mesh_face_scan, tsdf_mesh_face_scatter.
 * At most 2048 workgroups per launch, each striding over the tiles beyond.  No atomics, no workgroup waits on another,
 * no host synchronisation, no copy: the same bits on every run and on every stream.  origin[3] (host) finite,
 * voxel_size > 0 and finite, min_weight not NaN, capacities >= 0, 4-byte alignment; 7 * nx * ny * nz and
 * 12 * (nx - 1) * (ny - 1) * (nz - 1) <= 2^31 - 1.  No output may overlap an input, another output or the workspace.
 * workspace: pds_tsdf_mesh_workspace_bytes(nx, ny, nz) bytes (twice pds_tsdf_extract_workspace_bytes, plus 4 bytes per
 * voxel rounded up to 256, plus 1 byte per voxel rounded up to 256; 0 and an error message for a volume the entry point
 * refuses), 16-byte aligned, contents undefined before and after.  Out of scope: colour, sparse or hashed volumes,
 * simplification, welding of vertices across exact zeros, marching cubes proper.
 * ---------------------------------------------------------------------------------- */
size_t pds_tsdf_mesh_workspace_bytes(int nx, int ny, int nz);
int pds_tsdf_mesh_fwd(const float* tsdf, const float* weight, const float* origin /* host, [3] */, float voxel_size,
                      float min_weight, float* points, float* normals /* or NULL */, int* index /* or NULL */,
                      int* offsets /* [2] */, long long capacity, int* faces, int* face_offsets /* [2] */,
                      long long face_capacity, int nx, int ny, int nz, void* workspace, size_t workspace_bytes,
                      pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * TSDF raycast: the volume seen from a pinhole camera, as depth and normals         not in the reference
 * Additive: ABI version unchanged.  The other half of KinectFusion: the model prediction at a pose, and N noisy frames
 * as one clean depth map.  tsdf, weight: the volume of pds_tsdf_integrate_fwd, read only.  In grid coordinates voxel
 * (i, j, k) is the point (i, j, k).  rays [batch][12] (host): per entry M (3 x 3, row-major) then o (3): a point p of the
 * camera frame lies at the grid position M p + o (the Python mirror: M = R^T / voxel_size,
 * o = (-R^T t - origin) / voxel_size - 0.5 for the pose [R | t] from the world into the camera frame; fp64, rounded
 * once).  rotations [batch][9] (host): R.  camera[5] = fx, fy, cx, cy, skew.  Per pixel (px, py), in fp32, every
 * multiply-add an fmaf:
 *   1. y = (py - cy) / fy, x = ((px - cx) - skew y) / fx, dir = (x, y, 1): the ray parameter s IS the camera Z.
 *      d = M dir, g(s) = o + s d
 *   2. [s0, s1]: s clipped to 0 <= g_a <= n_a - 1 on the three axes (slabs) and to [near, far]; a miss if that is empty or
 *      not finite or if any n_a < 2
 *   3. samples s_m = fmaf(m, step, s0), m = 0, 1, ... while s_m <= s1; c_a = min(floor(g_a), n_a - 2) (not below 0),
 *      f_a = g_a - c_a; the sample is observed iff the eight corners of cell c have weight >= min_weight; its value is
 *      then the trilinear interpolant of tsdf, in x, then y, then z, each lerp fmaf(t, b - a, a)
 *   4. the march stops at the first observed sample whose value is < 0: a hit iff sample m - 1 exists, is observed and is
 *      not < 0; otherwise, and past s1, a miss
 *   5. depth = fmaf(step, v_prev / (v_prev - v_cur), s_prev)
 *   6. normal = the analytic gradient of the trilinear interpolant in the cell that contains g(depth), rotated by R,
 *      scaled by its largest component and normalised; (NaN, NaN, NaN) where that cell has an unobserved corner or the
 *      gradient is zero or not finite; the depth stays.  The tsdf is positive towards the camera, so the normal faces it;
 *      where the rotated gradient points along the ray instead (its dot product with dir is > 0) it is negated.
 * depth [batch, h, w] fp32: the camera-frame Z along the ray of the pixel centre, NaN at a miss (the convention of
 * pds_reproject_fwd's depth).  normals [batch, h, w, 3] fp32, nullable.  voxel_size > 0 and finite: it serves one check
 * only, that the box diagonal in metres / step is at most 65536 samples (|dir| >= 1: no ray has more; the kernel's loop
 * is bounded besides).  step > 0 and finite, 0 <= near < far (far may be inf), min_weight not NaN, fx, fy > 0, camera,
 * rays and rotations finite, batch * h * w <= 2^31 - 1, 4-byte alignment.  No output may overlap the volume or the other
 * output.  One launch per 16 batch entries (tsdf_raycast): one thread per pixel, a workgroup per 16 x 16 pixel tile, each
 * wave an 8 x 8 block of it; batch * ceil(h / 16) * ceil(w / 16) workgroups.  No workspace, no atomics, no workgroup
 * waits on another, no host synchronisation: the same bits on every run and on every stream.  Out of scope: empty-space
 * skipping that changes the sample positions, refinement beyond the one linear step, colour, a sparse volume, pose
 * estimation.
 * ---------------------------------------------------------------------------------- */
int pds_tsdf_raycast_fwd(const float* tsdf, const float* weight, int nx, int ny, int nz, float voxel_size,
                         const float* rays /* host, [batch][12] */, const float* rotations /* host, [batch][9] */,
                         const float* camera /* host, [5] */, float step, float z_near, float z_far, float min_weight,
                         float* depth, float* normals /* or NULL */, int batch, int h, int w, pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * TSDF colour: coloured integration, the colours of the extracted surface and of a raycast    not in the reference
 * Additive: ABI version unchanged.  The fused model keeps the image (KinectFusion, Open3D TSDFVolume with colour).  Beside
 * tsdf and weight of pds_tsdf_integrate_fwd the caller holds color, fp32 [nz, ny, nx, 3], interleaved (voxel v owns
 * color[3 v .. 3 v + 2]), 0 in a fresh volume.  The colour shares the weight: it has none of its own, so every frame is
 * integrated with its image.
 *
 * pds_tsdf_color_integrate_fwd.  The arguments of pds_tsdf_integrate_fwd, and image: the picture of every entry,
 * image_layout 0: fp32 [batch, 3, h, w], 1: uint8 [batch, h, w, 3] (the two layouts of pds_point_cloud_fwd and
 * pds_remap_fwd); the values are taken as they are, not rescaled.  Per entry the same two launches: tsdf_depth itself,
 * then tsdf_color_integrate, which makes per voxel the decisions of tsdf_integrate, steps 1 to 9 there, through the same
 * device functions: tsdf and weight receive the bits pds_tsdf_integrate_fwd gives them.  It adds one step: where the voxel
 * is updated, for c = 0, 1, 2, with x the image value of channel c at the pixel (px, py) the Z was read from and W_old the
 * weight before step 9:
 *     color[3 v + c] = fmaf(color[3 v + c], W_old, x * wt) / (W_old + wt)
 * (Open3D's rule: the colour is updated wherever the tsdf is.)  A skipped voxel is neither read nor written in any of the
 * three tensors.  The walk is tsdf_integrate's: quads of four consecutive voxels on a 16-byte boundary of tsdf and weight,
 * 256 threads, a grid-stride loop over at most 2048 workgroups; a fully updated quad takes its 12 colour floats as three
 * 16-byte accesses where color + 3 * (the quad's first voxel) is 16-byte aligned, and voxel by voxel otherwise.  Every
 * multiply-add is an fmaf: the same bits in every form, on every run and on every stream; no atomics, no workgroup waits
 * on another, no host synchronisation.  The conditions of pds_tsdf_integrate_fwd hold; image_layout is 0 or 1; 4-byte
 * alignment of color (and of a fp32 image); tsdf, weight, color and the workspace may not overlap one another or an
 * input.  workspace: pds_tsdf_integrate_workspace_bytes(h, w) bytes, 16-byte aligned.
 *
 * pds_tsdf_color_gather_fwd.  The colours of the rows an extraction wrote.  index [capacity] int32 and offsets [2] int32
 * (device) as pds_tsdf_extract_fwd (edges_per_voxel = 3: index = 3 v + a, d = 1 << a) or pds_tsdf_mesh_fwd
 * (edges_per_voxel = 7: index = 7 v + (d - 1)) wrote them.  For every row below min(offsets[1], capacity):
 *     n = v + offset(d), r = tsdf[v] / (tsdf[v] - tsdf[n]) (the expression the point was placed with), and for c = 0, 1, 2
 *     colors[3 row + c] = fmaf(r, color[3 n + c] - color[3 v + c], color[3 v + c])
 * colors [capacity, 3] fp32.  Rows beyond the count are not written.  A row whose index is negative or whose n lies beyond
 * the last voxel (nothing an extraction writes) gets (NaN, NaN, NaN) and reads nothing.  One launch (tsdf_color_gather):
 * one lane per output float, a grid-stride loop over at most 2048 workgroups of 256 threads, contiguous stores; the count
 * is read on the device: no host synchronisation, no atomics.  edges_per_voxel is 3 or 7; edges_per_voxel * nx * ny * nz
 * <= 2^31 - 1; capacity >= 0; 4-byte alignment.  colors may not overlap an input.
 *
 * pds_tsdf_color_render_fwd.  The colour of a raycast.  depth [batch, h, w] fp32 as pds_tsdf_raycast_fwd wrote it for
 * the same rays, camera and min_weight.  One thread per pixel (tsdf_color_render; the 16 x 16 tiles of tsdf_raycast, one
 * launch per 16 entries), in fp32:
 *     g = o + depth * d, with d and o of step 1 there (the same device function)
 *     the cell c_a = min(floor(g_a), n_a - 2) (not below 0), f_a = g_a - c_a
 *     colors[pixel][c] = the trilinear interpolant of channel c over the cell's eight corners, in x, then y, then z, each
 *     lerp fmaf(t, b - a, a)
 * (NaN, NaN, NaN) where depth is NaN, where a corner has weight < min_weight (the rule of the normal: colour and normal
 * exist at the same pixels, except where the gradient is zero) or where any n_a < 2.  colors [batch, h, w, 3] fp32.
 * min_weight not NaN, fx, fy > 0, camera and rays finite, batch * h * w <= 2^31 - 1, 4-byte alignment.  colors may not
 * overlap an input.  No workspace, no atomics, no host synchronisation: the same bits on every run and on every stream.
 * Out of scope: a colour term in ICP, a colour weight of its own, colour only inside the truncation band, uint8 storage,
 * sparse volumes.
 * ---------------------------------------------------------------------------------- */
int pds_tsdf_color_integrate_fwd(const float* disparity, const unsigned char* valid /* or NULL */,
                                 const float* confidence /* or NULL */, float min_confidence, int weight_by_confidence,
                                 const void* image, int image_layout, const float* matrix /* host, [16] */,
                                 const float* transforms /* host, [batch][12] */, const float* camera /* host, [5] */,
                                 float truncation, float max_weight, float* tsdf, float* weight, float* color,
                                 int nx, int ny, int nz, int batch, int h, int w,
                                 void* workspace, size_t workspace_bytes, pds_stream_t stream);
int pds_tsdf_color_gather_fwd(const int* index, const int* offsets /* [2] */, int edges_per_voxel, const float* tsdf,
                              const float* color, float* colors, long long capacity, int nx, int ny, int nz,
                              pds_stream_t stream);
int pds_tsdf_color_render_fwd(const float* weight, const float* color, int nx, int ny, int nz,
                              const float* rays /* host, [batch][12] */, const float* camera /* host, [5] */,
                              float min_weight, const float* depth, float* colors, int batch, int h, int w,
                              pds_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Frame-to-model tracking: the point-to-plane ICP system of a disparity frame against a raycast    not in the reference
 * Additive: ABI version unchanged.  The consumer of pds_tsdf_raycast_fwd's model prediction.  disparity [batch, h, w]
 * fp32; valid / confidence / min_confidence / matrix as pds_reproject_fwd takes them; normals [batch, h, w, 3] fp32,
 * nullable: the frame's normals as pds_surface_normals_fwd writes them (NaN: none).  model_depth [model_batch, hm, wm] and
 * model_normals [model_batch, hm, wm, 3] fp32 as pds_tsdf_raycast_fwd writes them, model_batch == batch or 1.
 * camera[5] = fx, fy, cx, cy, skew of the model's pinhole.  transforms [batch][12] (host): per entry R (3 x 3, row-major)
 * then t, from the frame's camera into the model's (fp64 on the host, rounded once).  Per source pixel, in fp32, every
 * multiply-add an fmaf:
 *   1. P = the point pds_reproject_fwd gives (the same device function); no row where it is NaN
 *   2. q_a = fmaf(R_a0, P_x, fmaf(R_a1, P_y, fmaf(R_a2, P_z, t_a))); no row unless q_z > 0 and q is finite
 *   3. x = q_x / q_z, y = q_y / q_z, u = fmaf(fx, x, fmaf(skew, y, cx)), v = fmaf(fy, y, cy), px = floor(u + 0.5),
 *      py = floor(v + 0.5) (the rounding of pds_register_depth_fwd and pds_tsdf_integrate_fwd); no row outside
 *      [0, wm) x [0, hm)
 *   4. Z = model_depth[py, px], n = model_normals[py, px]; no row where either holds a NaN.  y_m = (py - cy) / fy,
 *      x_m = fmaf(-skew, y_m, px - cx) / fx (the ray of pds_tsdf_raycast_fwd), m = (Z x_m, Z y_m, Z)
 *   5. e = m - q; no row unless fmaf(e_x, e_x, fmaf(e_y, e_y, e_z e_z)) <= max_distance * max_distance
 *   6. with normals: s = R n_f, each component fmaf(R_a0, n_fx, fmaf(R_a1, n_fy, R_a2 n_fz)); no row where n_f holds a
 *      NaN or not fmaf(s_x, n_x, fmaf(s_y, n_y, s_z n_z)) >= min_cosine
 *   7. r = fmaf(n_x, e_x, fmaf(n_y, e_y, n_z e_z)), J = (q x n, n), (q x n)_x = fmaf(q_y, n_z, -(q_z n_y)) and cyclic.
 *      The row is the seven fp32 values (J_0 .. J_5, r).
 * system [batch][29] fp64 (4-byte alignment suffices): the upper triangle of sum J J^T (21, row-major), sum J r (6),
 * sum r^2, the row count.  Each product is formed exactly in fp64 from the fp32 row values and added in fp64, in a fixed
 * order: icp_rows, one workgroup of 256 threads per tile of 1024 source pixels of one entry (thread t takes pixels
 * tile * 1024 + k * 256 + t, k = 0 .. 3; the wave folds lane + 32, + 16, ... + 1; waves 0 .. 3 in order) stores one
 * partial of 29 doubles per workgroup into the workspace, one launch per 16 entries; icp_reduce, one workgroup per entry,
 * adds the partials in ascending tile order.  No atomics, no workgroup waits on another, no host synchronisation: the
 * same bits on every run and on every stream.  rows [batch, h, w, 7] fp32, nullable: the row of every pixel, seven NaNs
 * where there is none.  max_distance > 0 and finite, min_cosine not NaN, fx, fy > 0, camera, matrix and transforms
 * finite, batch * h * w and model_batch * hm * wm <= 2^31 - 1, 4-byte alignment.  No output may overlap an input or
 * another output.  workspace: pds_icp_workspace_bytes(batch, h, w) bytes (232 per tile of 1024 pixels and entry, rounded
 * up to 256; 0 and an error message for a shape the entry point refuses), 8-byte aligned, contents undefined before and
 * after.  Out of scope: colour terms.  (Huber weights and the disparity pyramid: pds_hip_tracking.h.)
 * ---------------------------------------------------------------------------------- */
size_t pds_icp_workspace_bytes(int batch, int h, int w);
int pds_icp_system_fwd(const float* disparity, const unsigned char* valid /* or NULL */,
                       const float* confidence /* or NULL */, float min_confidence, const float* matrix /* host, [16] */,
                       const float* normals /* or NULL */, const float* model_depth, const float* model_normals,
                       int model_batch, int hm, int wm, const float* camera /* host, [5] */,
                       const float* transforms /* host, [batch][12] */, float max_distance, float min_cosine,
                       double* system, float* rows /* or NULL */, int batch, int h, int w, void* workspace,
                       size_t workspace_bytes, pds_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PDS_HIP_H */
