/* mww.h — C ABI of libmww_hip.so: the MI355X-native (gfx950) train-step engine for
 * microWakeWord's MixedNet and Inception classifiers.
 *
 * The reference (kahrendt/microWakeWord) has no FFI layer: its hot path is duck-typed Python
 * (microwakeword/train.py:249-299) calling numpy batch assembly (microwakeword/data.py:497-597)
 * and Keras `train_on_batch` on the graph built by microwakeword/mixednet.py:278-386 or
 * microwakeword/inception.py:232-340.  This
 * header is the boundary a maintainer would bind (ctypes / cffi / pybind — see INTEGRATION.md):
 * plain pointers and sizes, no torch / Python types.  Each entry point names the reference
 * interface it replaces.
 *
 * Conventions: every call returns MWW_OK (0) or a negative error code; the message is available
 * from mww_last_error() (thread-local).  The caller owns every host pointer; the library owns
 * all device memory.  A context is bound to one device and one HIP stream and is NOT thread
 * safe (one context per rank, one host thread).  Calls enqueue work on the context's stream;
 * only the mww_read_* / mww_get_* / mww_synchronize calls wait for the device.
 */
#ifndef MWW_H
#define MWW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MWW_OK 0
#define MWW_ERR_INVALID -1      /* bad argument / unsupported configuration */
#define MWW_ERR_HIP -2          /* a HIP runtime call failed */
#define MWW_ERR_UNSUPPORTED -3  /* model shape has no compiled kernel instantiation (mww_create: fall back to mww_create_convnet) */
#define MWW_ERR_STATE -4        /* call sequence error (e.g. train step before a batch) */

#define MWW_MAX_BLOCKS 8
#define MWW_MAX_STORES 64
#define MWW_FEATURE_BINS 40

typedef struct mww_ctx mww_ctx;

/* ---- model: replaces mixednet.model(flags, shape, batch_size) (mixednet.py:278-386) with the specialised
 * MFMA block kernels.  Covers conv1 -> ReLU -> n x [MixConv + 1x1 + BN + ReLU] -> Flatten -> Dense for the
 * (filters, kernel size) shapes instantiated in csrc/mww_lib.hip; every other flag combination (repeat_in_block,
 * residual_connection, spatial_attention, pooled, other widths ...) is expressed as a mww_convnet_desc below.
 * `block_kernel[i]` is the aligned depthwise length of block i (= the LAST listed MixConv kernel
 * size, mixednet.py:227); smaller MixConv groups are expressed by the host as zero leading taps
 * plus a gradient mask (mww_set_grad_mask), SURVEY §A.2.
 * Flat trainable-parameter order ("native order" == Keras get_weights() order without the BN
 * moving statistics):
 *   conv1.kernel[K1*40*C1] ; per block: dw.kernel[K*Cin] dw.bias[Cin] pw.kernel[Cin*Cout]
 *   bn.gamma[Cout] bn.beta[Cout] ; dense.kernel[T_last*C_last] dense.bias[1]
 * BN state order: per block moving_mean[Cout] moving_variance[Cout]. */
typedef struct {
  int32_t frames;               /* T: spectrogram_length (model_train_eval.py:82-88) */
  int32_t conv1_filters;        /* --first_conv_filters  (mixednet.py:76-81) */
  int32_t conv1_kernel;         /* --first_conv_kernel_size */
  int32_t conv1_stride;         /* --stride: time stride of the first convolution */
  int32_t n_blocks;
  int32_t block_filters[MWW_MAX_BLOCKS];  /* --pointwise_filters */
  int32_t block_kernel[MWW_MAX_BLOCKS];   /* max/last of --mixconv_kernel_sizes per block */
  int32_t max_batch;            /* largest batch any call will use */
} mww_mixednet_desc;

const char* mww_version(void);
const char* mww_last_error(void);
int mww_device_count(void);

/* 1 if every block of `desc` has a specialised MFMA block kernel (bf16 != 0: in the bf16 modes too), 0 if the model has to
 * run on the conv / depthwise graph kernels of mww_create_convnet (mww_last_error() says which block is not covered, or that the
 * classifier head holds fewer final frames than the model has: 768 / 504 / 384 at 32 / 48 / 64 channels).
 * Needs no device: it answers from the build-time shape table (csrc/block_launch.hip.h).  mww_create refuses the same shapes
 * with MWW_ERR_UNSUPPORTED. */
int mww_block_kernels_cover(const mww_mixednet_desc* desc, int bf16);

/* stream: a hipStream_t to run on (e.g. torch.cuda.current_stream().cuda_stream) or NULL for a
 * private non-blocking stream. */
int mww_create(const mww_mixednet_desc* desc, int device, void* stream, mww_ctx** out);

/* ---- conv -> BN/SSN -> ReLU graphs: replaces inception.model(flags, shape, batch_size)
 * (microwakeword/inception.py:232-340) and its building blocks conv2d_bn / conv2d_bn_delay (:46-141:
 * Conv2D(k x 1, dilation, valid, use_bias=False) -> BatchNormalization or SubSpectralNormalization
 * (layers/sub_spectral_normalization.py:49-61: channel c uses slot c % groups) -> ReLU) and the
 * three-branch block's StridedDrop + Concatenate (:143-209; strided_drop.py:42 drops LEADING frames).
 * The head is Flatten -> Dropout(rate) -> Dense(1, sigmoid) (:330-338) on the LAST op.
 * Ops are listed in layer-creation order, so the flat parameter vector is Keras get_weights() order:
 *   per op: kernel[k*Cin*filters] (depthwise: [k*filters]) then gamma[slots] beta[slots] (MWW_NORM_BN) or
 *   bias[filters] (MWW_NORM_BIAS) ; dense.kernel[T_last*C_last] dense.bias[1]
 *   (slots = bn_groups if bn_groups > 1 else filters); BN state: per BN op moving_mean[slots] moving_variance[slots].
 * Every other entry point of this header works on such a context exactly as on a MixedNet one. */
#define MWW_MAX_GRAPH_OPS 48
#define MWW_MAX_OP_SOURCES 3
typedef struct {
  int32_t n_src;                        /* inputs concatenated along channels, in this order */
  int32_t src[MWW_MAX_OP_SOURCES];      /* producing op (index < this op's) or -1 for the spectrogram */
  int32_t src_drop[MWW_MAX_OP_SOURCES]; /* leading frames of that input dropped to align the branches */
  int32_t src_c0[MWW_MAX_OP_SOURCES];   /* first channel of the slice of that input this op reads ... */
  int32_t src_cn[MWW_MAX_OP_SOURCES];   /* ... and its width (0 = the whole tensor).  Sibling convolutions that read
                                           the same input (Inception's three 1x1 branch heads) can be fused by the caller
                                           into one op with the concatenated filters; each consumer then names its slice.
                                           The slices different consumers take from one producer must be identical or
                                           disjoint and together cover all of its channels. */
  int32_t kernel, dilation, filters;
  int32_t bn_groups;                    /* 1 = BatchNormalization, g > 1 = SubSpectralNormalization(g) */
  /* the four fields below default to 0 = the Inception vocabulary (dense conv, stride 1, BN/SSN, ReLU); the others
   * express any MixedNet flag combination the specialised block kernels do not cover (mixednet.py:307-360:
   * first conv with --stride and no BN, MixConv depthwise + bias with no activation, repeat_in_block > 1, ...) */
  int32_t kind;                         /* MWW_OP_CONV: k x 1 convolution over all input channels;
                                           MWW_OP_DEPTHWISE: per-channel k x 1 taps [k][C] (one source, filters == its channels) */
  int32_t stride;                       /* time stride (0/1 = none); only for ops fed by the spectrogram */
  int32_t norm;                         /* MWW_NORM_BN (gamma, beta + moving statistics), MWW_NORM_BIAS (bias[filters]), MWW_NORM_NONE */
  int32_t act;                          /* MWW_ACT_RELU or MWW_ACT_LINEAR */
  int32_t residual;                     /* 1 + index of an earlier conv + BN + linear op whose normalised output is added to
                                           this op's normalised output before the activation (mixednet.py:340-358); 0 = none */
  int32_t residual_drop;                /* leading frames of that op dropped to align it (StridedDrop) */
} mww_conv_bn_op;
#define MWW_OP_CONV 0
#define MWW_OP_DEPTHWISE 1
#define MWW_NORM_BN 0
#define MWW_NORM_BIAS 1
#define MWW_NORM_NONE 2
#define MWW_ACT_RELU 0
#define MWW_ACT_LINEAR 1
typedef struct {
  int32_t frames;
  int32_t n_ops;
  mww_conv_bn_op ops[MWW_MAX_GRAPH_OPS];
  float dropout;                        /* --dropout (inception.py:330), active in the train step only */
  int32_t max_batch;
  /* MixedNet's optional heads (mixednet.py:234-275,362-384), applied to the last op's activations when more than one
   * frame remains; both 0 = Flatten -> Dense.  With attention the flat parameter vector carries the attention
   * kernel[4*2] (Keras [4,1,2,1]) between the last op and dense.kernel. */
  int32_t head_attention;               /* --spatial_attention: SpatialAttention(kernel_size = 4) */
  int32_t head_pool;                    /* --pooled: 0 none, 1 average (AveragePooling2D), 2 max (--max_pool) over the remaining frames */
} mww_convnet_desc;
int mww_create_convnet(const mww_convnet_desc* desc, int device, void* stream, mww_ctx** out);
/* Dropout keep decisions for the next train steps, [B][T_last*C_last] bytes (0 = dropped); NULL
 * returns to the built-in counter-based generator (mww_set_option "dropout_seed").  Keras draws the
 * mask from a generator that cannot be reproduced outside TensorFlow, so parity tests inject it. */
int mww_set_dropout_mask(mww_ctx* ctx, const uint8_t* keep, int B);
void mww_destroy(mww_ctx* ctx);
int mww_synchronize(mww_ctx* ctx);

int64_t mww_num_params(const mww_ctx* ctx);    /* trainable scalars (22177 for default mixednet) */
int64_t mww_num_bn_state(const mww_ctx* ctx);  /* moving mean/variance scalars (384) */

/* ---- weights: replace model.get_weights()/set_weights()/save_weights()/load_weights()
 * (train.py:336-338,391-399,448-450; model_train_eval.py:420-426) at the array level. */
int mww_set_params(mww_ctx* ctx, const float* host, int64_t n);
int mww_get_params(mww_ctx* ctx, float* host, int64_t n);
int mww_set_bn_state(mww_ctx* ctx, const float* host, int64_t n);
int mww_get_bn_state(mww_ctx* ctx, float* host, int64_t n);
int mww_set_grad_mask(mww_ctx* ctx, const float* host_mask01, int64_t n);
/* optimizer slots of tf.keras.optimizers.Adam (train.py:207): m, v and the iteration count;
 * replaces the tf.train.Checkpoint(optimizer=...) payload of train.py:229-233 */
int mww_set_opt_state(mww_ctx* ctx, const float* m, const float* v, int64_t n, int64_t step);
int mww_get_opt_state(mww_ctx* ctx, float* m, float* v, int64_t n, int64_t* step);
int mww_get_grads(mww_ctx* ctx, float* host, int64_t n);  /* flat gradient of the last step */

/* ---- quantization-aware training of the weights.  The int8 streaming family quantizes every kernel symmetrically, narrow
 * range, one scale per output channel, ties away from zero: scale_c = max|w_c| / 127 (1 for an all-zero channel),
 * q = clamp(round(w / scale_c), -127, 127).  That grid is a function of the weights alone, so it can be imposed in the step:
 * with the option weight_qat = 1 (set through the option call below; default 0) every forward and backward launch reads a
 * shadow of the parameter vector in which each weight channel holds q * scale_c, refreshed from the master at the start of
 * every call that runs a forward (train step, forward, window evaluation; one more node of a captured step).  Adam, the
 * parameter / optimizer-state calls above and checkpoints keep addressing the fp32 master; the flat gradient is the one taken
 * at the shadow (straight-through estimator).  Activations are not fake-quantized.
 *
 * The channel map says which parameters form a channel, in CSR form: channel c owns the parameter indices
 * chan_elem[chan_start[c] .. chan_start[c + 1]), chan_start[0] = 0, chan_start[n_channels] = n_elems.  Parameters outside every
 * channel (biases, BN gamma / beta, structurally masked taps) are copied through, as is a channel whose maximum is not
 * finite.  The map is validated - indices in [0, P), no element in two channels, chan_start ascending - and a refused map
 * (MWW_ERR_INVALID) leaves the context as it was.  n_channels = 0 removes the map and turns the option off; setting the
 * option to 1 without a map is MWW_ERR_INVALID. */
int mww_set_weight_qat(mww_ctx* ctx, const int32_t* chan_start, const int32_t* chan_elem, int32_t n_channels, int64_t n_elems);
/* the parameter vector the next forward would read: the shadow of the current master, or the master with the option off */
int mww_get_forward_params(mww_ctx* ctx, float* host, int64_t n);

/* ---- weight averaging: an exponential moving average of the trainable parameters, kept on the device next to the master.
 * State: ema[P] in fp32, laid out and indexed like the vector of mww_get_params, and a count of the updates it has taken.
 * One update, with om = 1 - decay formed in double:
 *     updates == 0:  ema[i] = w[i]                                                         (a bit copy of the master)
 *     otherwise:     ema[i] = (float)((double)ema[i] + om * ((double)w[i] - (double)ema[i]))
 * three float64 operations and one rounding, uncontracted; a non-finite master propagates.  The update is enqueued on the
 * context's stream directly behind every Adam update - the one inside mww_train_step or mww_apply_gradients - after which the
 * optimizer step count is a multiple of every_steps (one more node of a captured step).  A step with MWW_STEP_NO_APPLY
 * updates nothing; mww_set_params does not touch the average.  The BatchNorm moving statistics are not trainable and are
 * not averaged: they are re-estimated for the average by the calls of the next block.
 *
 * mww_set_weight_ema installs the average (updates = 0) with decay in (0, 1) and every_steps >= 1; decay == 0 removes it and
 * frees the vector.  Other values are MWW_ERR_INVALID and leave the context as it was.
 *
 * With the option ema_forward = 1 (the option call below; default 0; MWW_ERR_INVALID without an installed average) and
 * once updates > 0, every non-training forward - mww_forward(training = 0), mww_evaluate_windows, mww_get_forward_params -
 * stands on the average instead of the master, with the master's current moving statistics - or, while they are valid, with
 * the average's own re-estimated ones (next block); with weight_qat it reads fake_quant(average).  mww_train_step and
 * mww_forward(training = 1) always read the master (or its shadow). */
int mww_set_weight_ema(mww_ctx* ctx, double decay, int64_t every_steps);
/* the average and its update count, for checkpoints (host may be NULL to read the count alone); n = mww_num_params */
int mww_get_ema_state(mww_ctx* ctx, float* host, int64_t n, int64_t* updates);
int mww_set_ema_state(mww_ctx* ctx, const float* host, int64_t n, int64_t updates);

/* ---- BatchNorm statistics for the average.  The moving statistics were accumulated under the raw iterates; the averaged
 * model wants the statistics of its own activations.  State: ema_bn[S] in fp32, laid out and indexed like the vector of
 * mww_get_bn_state, and a validity flag.  A pass over K >= 1 batches:
 *     batch k:  the forward of mww_forward(training = 1, update_metrics = 0) on the current batch - batch statistics, moving
 *               statistics untouched, no loss, no metrics, no dropout - reading the AVERAGE (with weight_qat:
 *               fake_quant(average)), whatever the ema_forward option says; directly behind it one collect launch adds, for
 *               every statistic slot s (a BN channel, a (channel, sub-band) slot of a SubSpectralNormalization), the fp32
 *               batch mean and biased batch variance that forward normalised with to float64 sums:
 *               M[s] += (double)mean_k[s], V[s] += (double)var_k[s], in batch order
 *     commit:   ema_bn[o_mm + s] = (float)(M[s] / (double)K), ema_bn[o_mv + s] = (float)(V[s] / (double)K); valid = 1
 * mean_k / var_k are re-derived from the sums the forward's own statistics fold consumed, with its expressions and summation
 * order: they are that fold's floats bit for bit.  No atomics: two passes over the same batches write the same bytes.  The
 * master's bn_state is never written, nothing random is drawn, and a pass is never captured under "graphs" (captured steps
 * stay replayable behind it).  While valid, every non-training forward that stands on the average (ema_forward = 1, updates
 * > 0) folds ema_bn instead of the master's moving statistics.  Whatever changes what such a forward reads clears the flag -
 * an update of the average, mww_set_ema_state, mww_set_weight_ema, the weight_qat option or map - and closes a pass in
 * progress; evaluations then read the master's moving statistics again.
 *
 * mww_bn_reestimate_begin zeroes the sums (MWW_ERR_INVALID unless an average is installed and has taken an update);
 * mww_bn_reestimate_batch runs the forward + collect on the current batch's first B rows (MWW_ERR_STATE without an open pass
 * or a batch); mww_bn_reestimate_commit writes ema_bn (MWW_ERR_STATE with no batch collected).  mww_bn_reestimate_windows is
 * the three over a window list, gathered from the resident stores like mww_evaluate_windows: n must be a positive multiple
 * of batch (MWW_ERR_INVALID otherwise), so that every batch weighs the same.  A refused call leaves the context as it was. */
int mww_bn_reestimate_begin(mww_ctx* ctx);
int mww_bn_reestimate_batch(mww_ctx* ctx, int B);
int mww_bn_reestimate_commit(mww_ctx* ctx);
/* (mww_bn_reestimate_windows: declared behind mww_evaluate_windows, where mww_window is known) */
/* the statistics a forward at the average folds: ema_bn with *valid = 1, or the master's moving statistics with *valid = 0
 * (host / valid may be NULL); the setter installs ema_bn and marks it valid (data-parallel: the mean of the ranks' passes).
 * n = mww_num_bn_state; MWW_ERR_INVALID without an installed average. */
int mww_get_ema_bn_state(mww_ctx* ctx, float* host, int64_t n, int* valid);
int mww_set_ema_bn_state(mww_ctx* ctx, const float* host, int64_t n);

/* ---- sharpness-aware steps (SAM) and global-norm gradient clipping.  Both stand on one quantity, the sum of squares of the
 * whole flat gradient g (indexed like mww_get_grads) between the backward pass and Adam:
 *     S = sumsq(g): 1024 lanes; lane j = the float64 sum of (double)g[i] * (double)g[i] over i = j, j + 1024, ... ascending,
 *                   multiply and add uncontracted; S = ((s_0 + s_1) + s_2) + ... in lane order.  No atomics.
 * Sharpness-aware step, radius rho:  scale = rho / (sqrt(S) + 1e-12) in float64; w'[i] = w[i] + (float)(scale * (double)g[i]).
 * Clipping, threshold c:             k = c / max(sqrt(S), c) in float64 (max(r, c) = r > c ? r : c, so k is exactly 1.0 at or
 *                                    below the threshold and for a NaN S); g[i] = (float)(k * (double)g[i]) in place.
 * Nothing is screened: a non-finite gradient gives a non-finite w', and the call still returns MWW_OK.
 *
 * With a radius installed, mww_train_step without MWW_STEP_NO_APPLY enqueues:
 *   1. shadow refresh (weight_qat); forward in training mode - moving statistics updated, loss, metrics as the flags say -
 *      and backward without Adam: g(w);
 *   2. S of g(w) and the perturbation: the master becomes w', a bit copy of w is kept;
 *   3. shadow refresh again (weight_qat: the second pass reads fake_quant(w')); forward on the same batch with the same dropout
 *      mask, batch statistics of its own, moving statistics NOT updated, loss, no metrics; backward without Adam: g(w');
 *   4. the master restored from the bit copy (never by subtracting); S of g(w'); the clip if installed; Adam at w with g(w'),
 *      the hyper-parameters pushed once and the optimizer step count up by one; the weight-average update when one is due.
 * So: the BatchNorm moving statistics and the metric counters are those of the first pass; the dropout counter advances once
 * per step (a run's mask sequence is that of a plain run); mww_get_grads returns what Adam consumed; mww_read_outputs
 * returns the last forward's values, i.e. the second pass's.  With clipping alone the step is forward, backward without Adam,
 * S, clip, Adam - at or below the threshold the bytes of the plain step.  Clipping also stands in front of Adam in
 * mww_apply_gradients (it sees the gradient buffer as it is; grad_scale multiplies behind it).  A MWW_STEP_NO_APPLY step is
 * never sharpened or clipped.  Under "graphs" such a step is enqueued eagerly (the same bytes); installing or removing either
 * feature drops the captured steps.  A context that installs neither launches exactly what it launched before.
 *
 * mww_set_sharpness_aware: rho > 0 installs, 0 removes; mww_set_grad_clip likewise.  Any other value (negative, NaN, infinite)
 * is MWW_ERR_INVALID.  Both are single-device: installing either next to an exchange hook, or a hook (mww_set_allreduce_hook,
 * mww_allreduce_init) next to either, is MWW_ERR_UNSUPPORTED.  A refused call leaves the context as it was.
 * mww_get_grad_norms returns S of the last such step's first-pass gradient and of the gradient Adam consumed, before
 * clipping (clipping alone: the same number twice); it waits for the stream; either pointer may be NULL; MWW_ERR_STATE before
 * the first such step. */
int mww_set_sharpness_aware(mww_ctx* ctx, double rho);
int mww_set_grad_clip(mww_ctx* ctx, double global_norm);
int mww_get_grad_norms(mww_ctx* ctx, double* first_sumsq, double* final_sumsq);

/* ---- feature stores: replace the RaggedMmap page-cache reads of data.py:255-258.  A store is the
 * flat concatenation of its samples ([T_i][40], uint16 raw micro-frontend values or float32
 * already scaled), uploaded once and kept resident in HBM. */
#define MWW_DTYPE_U16 0
#define MWW_DTYPE_F32 1
int mww_upload_store(mww_ctx* ctx, int store_id, const void* host_data, int64_t n_elems, int dtype);

/* ---- batch assembly: replaces FeatureHandler.get_data("training") materialisation
 * (data.py:555-597: fixed_length_spectrogram :74-118, uint16->f32 * 0.0390625 :268-269,
 * spec_augment :32-71, final shuffle :591-597).  All random choices are made on the host
 * (mww_sample_training_batch) and arrive here as integers. */
typedef struct {
  int32_t store;      /* store id */
  int32_t pad_rows;   /* zero frames in front (left pad, data.py:107-113) */
  int32_t copy_rows;  /* frames copied */
  int32_t reserved;
  int64_t src_elem;   /* element offset of the first copied frame inside the store */
} mww_window;
/* masks: [B][n_time_masks + n_freq_masks][2] = (start, width); time masks first.
 * Defines x[B][T][40] float32 of the context's batch buffer.  With the "fused_input" option (the default) only the
 * descriptors are uploaded and the kernels that read the spectrogram gather from the stores (the specialised MixedNet
 * first-block kernels; the stem of a conv/BN graph when it is the static 5 x 40 shape of the default Inception and the
 * window has at most 200 frames); the buffer itself is filled when any other reader needs it (other graphs,
 * mww_get_batch, mww_debug_read "x", a batch reused after its mailbox slot has moved on). */
int mww_assemble_batch(mww_ctx* ctx, const mww_window* windows, const int32_t* masks, int B, int n_time_masks,
                       int n_freq_masks);
/* ready-made batch: the `x` argument of Keras train_on_batch / evaluate (train.py:295-299,50-58) */
int mww_set_batch(mww_ctx* ctx, const float* host_x, int B);
int mww_get_batch(mww_ctx* ctx, float* host_x, int B);
/* labels and per-sample weights (penalty_weight * class weight, train.py:288-293) */
int mww_set_targets(mww_ctx* ctx, const float* host_y, const float* host_w, int B);

/* ---- the train step: replaces model.train_on_batch (train.py:295-299): forward(training=True),
 * weighted Keras BCE, backward, Adam(lr), BN moving statistics, metric update.
 * flags: MWW_STEP_NO_APPLY stops after the flat gradient is assembled (data-parallel: all-reduce
 * mww_device_ptr(MWW_BUF_GRADS), then mww_apply_gradients). */
#define MWW_STEP_NO_APPLY 1
#define MWW_STEP_NO_METRICS 2
int mww_train_step(mww_ctx* ctx, int B, float learning_rate, int flags);
int mww_apply_gradients(mww_ctx* ctx, float learning_rate, float grad_scale);

/* ---- data-parallel exchange.  The caller owns the communicator (RCCL through
 * torch.distributed, one process per GPU); the library calls back whenever a buffer has to be summed
 * over the ranks.  The callback must ENQUEUE an in-place sum all-reduce of device_buf[0..n) (no host
 * synchronisation needed) and return 0.  `flags` says how the exchange is ordered:
 *   MWW_EXCHANGE_IN_ORDER  the reduced values are read by the next launch on the context's stream: the all-reduce has to
 *                          be complete, in stream order, when the callback's work is reached (e.g. a blocking-in-stream
 *                          dist.all_reduce issued while the context's stream is the current stream);
 *   MWW_EXCHANGE_DEFERRED  a finished gradient bucket: the all-reduce may run on the communicator's own stream next to
 *                          the backward kernels that follow (SURVEY §8e "two buckets ... overlaps the remaining backward
 *                          blocks"); it only has to be complete when the next MWW_EXCHANGE_FLUSH call returns its work;
 *   MWW_EXCHANGE_FLUSH     device_buf = NULL, n = 0: order the context's stream after every deferred exchange.
 *   sync_bn = 1: BatchNorm statistics are exchanged in every train step — per BN layer one all-reduce of
 *                (sum x, sum x^2) in the forward and one of (sum g, sum g*xhat) in the backward — so the W
 *                ranks normalise over the GLOBAL batch exactly like the single-device reference ("parity
 *                mode"; 2 x layers tiny all-reduces on the critical path, no hipGraph replay).
 *   sync_bn = 0: local-batch statistics ("throughput mode").
 *   reduce_grads = 1: mww_train_step also all-reduces the flat gradient through the callback and applies
 *                Adam to the rank average, i.e. it is the complete data-parallel step.  With the specialised MixedNet
 *                kernels and option "grad_buckets" 2 the gradient goes in two buckets: [dense + the last two
 *                blocks] as soon as their backward kernels are enqueued (deferred), the rest after the first block's
 *                (default 1 = one exchange after the backward pass: the faster schedule at world size 1, and the only
 *                one measured so far).
 * fn = NULL removes the hook. */
#define MWW_EXCHANGE_IN_ORDER 0
#define MWW_EXCHANGE_DEFERRED 1
#define MWW_EXCHANGE_FLUSH 2
typedef int (*mww_allreduce_fn)(void* user, float* device_buf, int64_t n, int flags);
int mww_set_allreduce_hook(mww_ctx* ctx, mww_allreduce_fn fn, void* user, int world_size, int sync_bn, int reduce_grads);

/* ---- the same exchange with RCCL called from the library (SURVEY 8b `mww_allreduce_init`, 8e): one process per GPU,
 * rank 0 obtains a unique id (ncclGetUniqueId) and hands its MWW_UNIQUE_ID_BYTES bytes to every rank by whatever channel
 * the launcher has (torch.distributed store / broadcast, MPI, a file); every rank then calls mww_allreduce_init, which
 * joins the communicator (collective: returns when all ranks have called it) and installs an internal exchange in place of
 * the callback above with reduce_grads = 1: in-order exchanges are ncclAllReduce calls on the context's stream, a deferred
 * bucket runs on a library-owned side stream ordered by events - no callback into the host language per step.
 * librccl.so is bound at run time (dlopen), so a single-GPU user needs no RCCL.  mww_allreduce_destroy leaves the
 * communicator (also done by mww_destroy). */
#define MWW_UNIQUE_ID_BYTES 128
int mww_allreduce_unique_id(void* out_id, int capacity);
int mww_allreduce_init(mww_ctx* ctx, int rank, int world_size, const void* unique_id, int sync_bn);
int mww_allreduce_destroy(mww_ctx* ctx);
/* ranks of the library-owned communicator as RCCL reports them (ncclCommCount); 0 without one: a bench line can state how
 * many GPUs really took part in its collectives. */
int mww_allreduce_world(mww_ctx* ctx);

/* ---- inference forward on the current batch: replaces model(x, training=...) /
 * model.evaluate's per-batch forward (train.py:50-58). training=1 uses batch statistics without
 * touching the moving averages. update_metrics=1 also accumulates the compiled metrics. */
int mww_forward(mww_ctx* ctx, int B, int training, int update_metrics);

/* ---- evaluation of a whole window list: replaces model.evaluate(x, y, batch_size=1024) over the result of
 * FeatureHandler.get_data(<validation / testing mode>) (train.py:42-58,75-96; the ambient sets arrive as the 100 ms-stride
 * windows of data.py:301-311).  `windows` / `labels` ([n]) are host arrays; the library walks them in batches of `batch`:
 * descriptor upload, gather from the HBM-resident stores, inference forward (moving statistics folded once for the whole
 * call), threshold / AUC / loss counters accumulated on the device (read them with mww_metrics_read).  One call per
 * evaluation instead of three per batch. */
int mww_evaluate_windows(mww_ctx* ctx, const mww_window* windows, const float* labels, int64_t n, int batch);
/* a BatchNorm re-estimation pass over a window list (see "BatchNorm statistics for the average" above) */
int mww_bn_reestimate_windows(mww_ctx* ctx, const mww_window* windows, int64_t n, int batch);

/* outputs of the last train step / forward (waits for the stream). Any pointer may be NULL. */
int mww_read_outputs(mww_ctx* ctx, int B, float* probs, float* logits, float* loss);

/* ---- metrics: the nine compiled Keras metrics of train.py:209-221 as raw cumulative counters;
 * the host derives accuracy/recall/precision/tp..fn@101/auc@200/loss from them. */
typedef struct {
  uint64_t hist101[2][101]; /* [label][bucket], bucket = ceil(p*100)-1 (Keras evenly spaced thresholds) */
  uint64_t hist200[2][200]; /* AUC buckets, ceil(p*199)-1 clamped at 0 */
  uint64_t n, correct, tp5, fp5, fn5, pos, neg;
  double bce_sum;           /* unweighted Keras BCE summed over samples */
} mww_metrics;
int mww_metrics_read(mww_ctx* ctx, mww_metrics* out);
int mww_metrics_reset(mww_ctx* ctx);

/* ---- device buffers for the host's collectives (torch.distributed over RCCL) */
#define MWW_BUF_PARAMS 0
#define MWW_BUF_GRADS 1
#define MWW_BUF_BN_STATE 2
#define MWW_BUF_X 3
#define MWW_HANDLE_STREAM 4   /* not a buffer: the hipStream_t the context enqueues on (to order foreign work against it) */
void* mww_device_ptr(mww_ctx* ctx, int which);

/* named internal tensors for parity tests ("p1".."p8" pre-BN block outputs, "g1".. gradients at
 * the BN outputs, "bn<k>" the folded BN rows of block k, "a0" = relu(conv1(x)) as the first block stored it, "dz", "x");
 * returns the element count or a negative error */
int64_t mww_debug_read(mww_ctx* ctx, const char* name, int B, float* host, int64_t capacity);

/* options: "graphs" (0/1 replay the step from a hipGraph), "grid_fwd", "grid_bwd", "grid_head", "grid_graph",
 * "dropout_seed", "pointwise_bf16" (0 = exact fp32 MFMA, the default; 1 = the MixedNet 1x1 convolutions and
 * their two backward contractions take bf16-rounded operands with fp32 accumulation — BASELINE configs[4]),
 * "storage_bf16" (1 = additionally the block outputs p_k and the stashed gradients g_k live in HBM as bf16, every sum
 * stays fp32 and is taken from the unrounded values; implies pointwise_bf16, cleared by pointwise_bf16 = 0),
 * "fused_input" (default 1: mww_assemble_batch uploads descriptors only and the kernels that read the spectrogram - the
 * specialised MixedNet first-block kernels, the gathering stem of the default Inception graph - gather / scale / mask their
 * rows from the stores; x is materialised on demand — same values),
 * "bn_inline" (default 1: BN sums travel in fp64 accumulator rows and are folded by their first consumer instead of
 * by finalize launches, in the MixedNet block kernels and in conv/BN graphs whose ops are convolutions with a BatchNorm (or
 * nothing) and depthwise ops with a bias (or nothing), without residual branches and attention / pooled heads; forced off by
 * the sync-BN exchange hook), "tail_roles" (default 1, with bn_inline: the dense-weight
 * gradient and the metric update ride in the gradient-assembly launch), "bce_from_logits" (default 1: the loss is the
 * logits form Keras 3 evaluates for a sigmoid output, 0: clipped probability form), "graph_role_split" (default 1, conv/BN
 * graph contexts with bn_inline: launches that hold several roles - twin ops, weight + data gradient - divide the launch's
 * workgroups between the roles; "graph_dgrad_share" = percent of an op's workgroups that form its data gradient, 10..90),
 * "grid_graph" (conv/BN graph contexts: 0 = default, with bn_inline every launch takes the
 * grid its own LDS tile and registers let the CUs hold - at most "graph_fwd_wg_per_cu" / "graph_bwd_wg_per_cu" workgroups per
 * CU, default 4 / 4; > 0 = that many workgroups per launch; without bn_inline one grid of 3 per CU, because a tensor's
 * partial statistics rows are shared by its launches),
 * "graph_frame_chunks" (conv/BN graph contexts with bn_inline: the 1x1 ops - and the forward convolution of any op - process
 * a window as up to 4 frame chunks with correspondingly smaller LDS tiles; 0 = off, 1 = automatic, 2..4 = that many; default 1 for graphs
 * with depthwise ops (MixedNet flag sets: -7 % step time measured), 0 for pure convolution graphs (Inception: +0.5 ... +8 %)),
 * "graph_static_shapes" (conv/BN graph contexts: 1 = ops whose shape - kernel length, sources' widths and row lengths - has a
 * compile-time instantiation use it, the default; 0 = the run-time-shape kernels for every op),
 * "graph_planar" (conv/BN graph contexts: 1 = a 30- / 48-filter op whose consumers all read one of its equal channel slices keeps its
 * tensors one plane per slice, the default; 0 = interleaved),
 * "bwd_wide" (default 1: the block backward kernels of square 48- / 64-wide blocks - and of stride-3 first blocks - as 512-thread
 * workgroups; 0 = 256 threads),
 * "conv1_x6" (default 1, stride-1 first convolutions: the conv1 weight gradient as six bf16 slice products per fp32 product on the
 * bf16 matrix pipe, fp32-grade; 0 = exact-fp32 MFMA), "conv1_x6_fwd" (default 0: the same form for the first convolution of the
 * forward kernel - measured slower), "bwd_first_wide" (default 0, with conv1_x6: the 512-thread form of the stride-1 first block's
 * backward kernel - measured equal),
 * "dp_commit_late" (fp32 backward kernels: 1 = the dp rows of a tile are committed to LDS - and requested again for the next tile -
 * behind the depthwise recompute, a phase after the input rows; 0 = both row groups in front of it; -1 = the default of each kernel
 * family, the order that won its A/B: 1 for the first and the middle blocks, 0 for the last block.  A schedule only: results are bit-identical either way),
 * "grad_buckets" (data-parallel step: 1 = one exchange after the backward pass, the default; 2 =
 * overlapped two-bucket gradient exchange), "assemble_split" (workgroups per window of the
 * assembly kernel), "side_stream", "profile", "profile_split", "ablate" (profiling switches) */
int mww_set_option(mww_ctx* ctx, const char* name, int64_t value);

/* per-kernel timing of the last N steps measured with HIP events on the context's stream:
 * enable with mww_set_option("profile", 1); names/ms are returned in launch order. */
int mww_profile_read(mww_ctx* ctx, char* names, int names_capacity, float* ms, int capacity);

/* ---- host sampler: replaces the RNG-consuming part of FeatureHandler.get_data("training")
 * (data.py:540-569,591-595) bit-exactly; see csrc/sampler.cpp. */
#define MWW_STRATEGY_RANDOM 0
#define MWW_STRATEGY_TRUNCATE_START 1
#define MWW_STRATEGY_TRUNCATE_END 2
#define MWW_STRATEGY_FIXED_RIGHT_CUTOFF 3
#define MWW_STRATEGY_NONE 4
typedef struct {
  int32_t n_providers;            /* providers that have training samples, reference order */
  const double* sampling_weight;  /* [n_providers] */
  const int32_t* strategy;        /* [n_providers] MWW_STRATEGY_* */
  const int64_t* set_offsets;     /* [n_providers+1] into the set_* arrays */
  const int32_t* set_store;       /* store id of each entry of feature_sets["training"] (shuffled order) */
  const int64_t* set_src_elem;    /* element offset of the sample inside its store */
  const int32_t* set_len;         /* frames of the sample */
  const int32_t* cutoff_offsets;  /* [n_providers+1] */
  const int32_t* cutoffs;         /* fixed_right_cutoffs, concatenated */
} mww_sampler_desc;
/* py_state / np_state: 624 MT19937 words + position (625 uint32), advanced in place.
 * out_order is the final np.random.shuffle permutation: output slot j of the batch is draw
 * out_order[j].  apply_order = 0 leaves windows/masks/provider/sample in DRAW order, 1 permutes them
 * into the final batch order.  default_strategy < 0 means "default" (per provider). */
int mww_sample_training_batch(const mww_sampler_desc* d, uint32_t* py_state, uint32_t* np_state, int B, int T, int tmax,
                              int tcount, int fmax, int fcount, int32_t default_strategy, int32_t apply_order,
                              mww_window* out_windows, int32_t* out_masks, int32_t* out_provider, int32_t* out_sample,
                              int32_t* out_order);
int mww_rng_selftest(uint32_t* state, int which, int n, double* out_real, uint32_t* out_int, uint32_t bound);

/* ---- batch prefetcher: the draws of FeatureHandler.get_data("training") for the NEXT steps made by a worker thread
 * while the launching thread enqueues the current one (the reference alternates get_data and train_on_batch on one
 * thread, train.py:276-299; at 0.3 ms per step the 0.16 ms the draws of 1024 windows take is most of the host's share).
 * The worker owns private copies of the two MT19937 streams (py_state / np_state: 625 words each, as above) and calls
 * mww_sample_training_batch(..., apply_order = 1) in sequence, so batch n is the batch the synchronous path draws from
 * those states with its n-th call.  provider_label / provider_weight: label and per-sample weight (penalty_weight x
 * class weight, train.py:288-293) of each provider's windows.  depth = batches drawn ahead (1..16).
 * Host-only objects: no device or context is involved until mww_assemble_prefetched. */
typedef struct mww_prefetcher mww_prefetcher;
int mww_prefetch_create(const mww_sampler_desc* d, const float* provider_label, const float* provider_weight,
                        const uint32_t* py_state, const uint32_t* np_state, int B, int T, int tmax, int tcount, int fmax,
                        int fcount, int32_t default_strategy, int depth, mww_prefetcher** out);
/* The same with class and penalty weights kept apart: the reference multiplies penalty[B] by class_weight(y)[B,1]
 * (microwakeword/train.py:288-293), a [B,B] matrix W[i,j] = penalty_j * cw(y_i) that Keras reduces against the [B] per-sample
 * losses.  provider_weight = penalty weights; provider_class_weight = class weight of each provider's label;
 * broadcast 0: w_j = penalty_j * cw_j (then identical to mww_prefetch_create with the products);
 *           1: w_j = penalty_j * mean_i cw_i over the batch ("keras_last_axis": the reference's arithmetic, the default of
 *              microwakeword_amd.train); 2: w_i = cw_i * mean_j penalty_j ("keras_first_axis").  Means in float64. */
int mww_prefetch_create_weighted(const mww_sampler_desc* d, const float* provider_label, const float* provider_weight,
                                 const float* provider_class_weight, int broadcast, const uint32_t* py_state,
                                 const uint32_t* np_state, int B, int T, int tmax, int tcount, int fmax, int fcount,
                                 int32_t default_strategy, int depth, mww_prefetcher** out);
/* waits for the next batch; the arrays ([B] windows, [B][tcount+fcount][2] masks, [B] labels / weights / provider /
 * index of the sample inside its provider's training set) stay valid until mww_prefetch_release.  Any pointer may be NULL. */
int mww_prefetch_acquire(mww_prefetcher* p, const mww_window** windows, const int32_t** masks, const float** labels,
                         const float** weights, const int32_t** provider, const int32_t** sample);
int mww_prefetch_release(mww_prefetcher* p);
/* the two streams as they stood after the last batch handed out (batches drawn ahead of it do not count): what the
 * synchronous sampler continues from when the prefetcher is dropped.  Returns the number of batches handed out. */
int64_t mww_prefetch_rng_state(mww_prefetcher* p, uint32_t* py_state, uint32_t* np_state);
int mww_prefetch_shape(const mww_prefetcher* p, int* B, int* n_time_masks, int* n_freq_masks);   /* as created */
void mww_prefetch_destroy(mww_prefetcher* p);
/* mww_prefetch_acquire + mww_set_targets + mww_assemble_batch + mww_prefetch_release in one call; out_labels /
 * out_weights ([B], may be NULL) receive copies of what went to the device. */
int mww_assemble_prefetched(mww_ctx* ctx, mww_prefetcher* p, float* out_labels, float* out_weights);

/* ---- streaming inference and detection metrics: replaces the evaluation that follows training in the reference
 * (model_train_eval.py:131-272 evaluate_model with --test_tflite_streaming / --test_tflite_nonstreaming;
 * test.py:293-403 tflite_streaming_model_roc; inference.py:82-125 Model.predict_spectrogram) without TensorFlow / TFLite.
 * A stream object borrows an existing context's device, HIP stream and uploaded feature stores (the context must outlive
 * it).  Topology: MixedNet with a first convolution, any widths / kernels / repeat_in_block - without residual connections,
 * spatial attention or pooled head through mww_stream_create, with them through mww_stream_create_mixednet below (spatial
 * attention in non_stream mode only); Inception - any conv/BN graph of mww_convnet_desc's Inception
 * vocabulary - through mww_stream_create_convnet below.  Weights arrive in Keras get_weights() order (BN moving statistics included), so the
 * same call serves the specialised-kernel and the generic-graph MixedNet contexts; BN is folded into the 1x1 weights.
 *   MWW_STREAM_MODE_STREAM: Modes.STREAM_INTERNAL_STATE_INFERENCE - every Stream layer keeps the last R frames of its
 *     input (zeros after create / reset; layers/stream.py:580-594), each `stride` frames fed yield one probability, the
 *     rings carry over from track to track and from call to call; the last L mod stride frames of a track are not fed.
 *   MWW_STREAM_MODE_NON_STREAM: the non-streaming model on the windows of `frames` rows ending at T, T + stride, ... <= L
 *     of every track, each scored on its own (a track shorter than T gives nothing). */
#define MWW_STREAM_MODE_STREAM 0
#define MWW_STREAM_MODE_NON_STREAM 1
#define MWW_STREAM_MAX_KERNELS 8
#define MWW_STREAM_MAX_REPEAT 8
typedef struct {
  int32_t conv1_filters, conv1_kernel, stride;            /* --first_conv_filters, --first_conv_kernel_size, --stride */
  int32_t n_blocks;
  int32_t repeat[MWW_MAX_BLOCKS];                         /* --repeat_in_block */
  int32_t n_kernels[MWW_MAX_BLOCKS];                      /* entries of each --mixconv_kernel_sizes list (ascending) */
  int32_t kernels[MWW_MAX_BLOCKS][MWW_STREAM_MAX_KERNELS];
  int32_t pointwise_filters[MWW_MAX_BLOCKS];              /* --pointwise_filters */
  int32_t t_final;                                        /* T_f: frames of the final map the Dense reads */
  int32_t frames;                                         /* T: window length of the non-streaming model (non_stream mode) */
  int32_t mode;                                           /* MWW_STREAM_MODE_* */
} mww_stream_desc;
typedef struct mww_stream mww_stream;
/* MWW_ERR_UNSUPPORTED (+ message) for a malformed description or a topology outside the list above */
int mww_stream_create(mww_ctx* ctx, const mww_stream_desc* desc, mww_stream** out);
/* The same handle for a MixedNet with residual connections, a pooled head or spatial attention (csrc/tu_stream.hip, the kernel's <VAR> form).
 * The description is the superset of mww_stream_desc; with no option set the stream is the one of mww_stream_create.  It is a
 * creator of its own because the test-suite pins what mww_stream_create takes and refuses: the old name keeps its behaviour.
 *   residual[b] (--residual_connection; mixednet.py:340-358): r = BN(Conv1x1(block input)), no bias, no ring and no state, is
 *     added to the BN output of EVERY repeat of block b before that repeat's ReLU, at the same position (the non-streaming
 *     graph's StridedDrop drops the residual's leading frames: right alignment; in stream mode both branches hold the current
 *     frame).  Keras order: b.res.kernel [1,1,Cin,F], gamma, beta, moving_mean, moving_variance in front of the block's repeats.
 *   pool (--pooled / --max_pool; mixednet.py:362-381): 0 none, 1 average, 2 max over the frames the head holds - in stream mode
 *     the head ring [T_f - 1][C] plus the current frame, cold-ring zeros included (the average divides by T_f from the first
 *     output on, the maximum includes 0) - then the Dense over the C pooled values.
 *   spatial_attention (--spatial_attention; mixednet.py:234-275), non_stream mode only: per final-map position the mean and
 *     the max over the channels, a[q] = sigmoid(sum_{i<4} w[i,0] avg[q-3+i] + w[i,1] max[q-3+i]), g[q] = h[q] a[q]; the Dense
 *     (or the pooling, then the Dense) reads the last T_f - 3 positions of g.  Keras order: attention.kernel [4,1,2,1] in front
 *     of the Dense.  Stream mode is refused: the reference's streaming clone gates the last T_f - 3 ring frames with the
 *     CURRENT attention value (by our reading), which is not this computation, and nothing available pins that reading.
 *   t_final: frames of the final map BEFORE attention and pooling; with t_final = 1 the head options do nothing (mixednet.py:362).
 *   The state layout is that of mww_stream_create (residuals add nothing).  The six int8 entry points return
 *   MWW_ERR_UNSUPPORTED on a stream whose description uses any of the three options.
 * MWW_ERR_UNSUPPORTED (+ message) at creation: attention with t_final < 4 or in stream mode, a t_final that does not match the
 * non_stream window, option values outside their range, everything mww_stream_create refuses. */
typedef struct {
  int32_t conv1_filters, conv1_kernel, stride;
  int32_t n_blocks;
  int32_t repeat[MWW_MAX_BLOCKS];
  int32_t n_kernels[MWW_MAX_BLOCKS];
  int32_t kernels[MWW_MAX_BLOCKS][MWW_STREAM_MAX_KERNELS];
  int32_t pointwise_filters[MWW_MAX_BLOCKS];
  int32_t t_final;                                        /* frames of the final map before attention and pooling */
  int32_t frames;
  int32_t mode;
  int32_t residual[MWW_MAX_BLOCKS];                       /* 0 / 1 per block */
  int32_t spatial_attention;                              /* 0 / 1 */
  int32_t pool;                                           /* 0 none, 1 average, 2 max */
} mww_mixednet_stream_desc;
int mww_stream_create_mixednet(mww_ctx* ctx, const mww_mixednet_stream_desc* desc, mww_stream** out);
/* The same MixedNet stream (same description, plan, float weights, state layout, same handle type) on which the six int8 entry
 * points work when the description uses residual or pool: calibration on the float kernel's <VAR, REC> form (csrc/tu_stream.hip), then
 * the int8 kernel's <VAR> form (csrc/tu_stream_q8.hip) once mww_stream_set_quantized has loaded parameters (layout: next to
 * mww_stream_set_quantized below; contract: INTEGRATION.md 6, "residual and pooled MixedNets").  A creator of its own for the
 * reason mww_stream_create_convnet_q8 gives: the refusal of the int8 calls on a stream of mww_stream_create_mixednet is pinned
 * by the test-suite (tests/mixednet_variant_checks.py).  spatial_attention is refused here in BOTH modes
 * (MWW_ERR_UNSUPPORTED naming it): the int8 model is a stream-mode model and int8 MUL / Logistic gating is not restated.  A
 * description with no option set, or with t_final = 1, is the plain plan on the plain kernels, as mww_stream_create. */
int mww_stream_create_mixednet_q8(mww_ctx* ctx, const mww_mixednet_stream_desc* desc, mww_stream** out);
/* The same handle for a conv -> BN/SSN -> ReLU graph: the streaming / non-streaming Inception model (inception.py:233-338 in
 * Modes.STREAM_INTERNAL_STATE_INFERENCE, one frame per step; csrc/tu_stream_graph.hip).  `desc` is the mww_convnet_desc of the
 * model with the ops in Keras layer-creation order (un-fused branch heads), `mode` a MWW_STREAM_MODE_*; `dropout` and
 * `max_batch` are not read.  Every mww_stream_* call below works on it unchanged, except the int8 ones (mww_stream_num_tensors,
 * _calibrate_host, _set_quantized, _q8_sizes, _read_q8, _get_state_q8), which return MWW_ERR_UNSUPPORTED with a message
 * ("... MixedNet streams only ...") on a stream of this creator; mww_stream_create_convnet_q8 below creates the graph stream
 * that takes them.
 *   vocabulary: MWW_OP_CONV, stride 0 / 1, MWW_NORM_BN (BatchNormalization or SSN groups), MWW_ACT_RELU, 1..3 sources with
 *     src_drop and channel slices, no residual, no head_attention / head_pool.  Anything else, sources that src_drop does not
 *     align, or a graph that does not fit `frames` is refused with MWW_ERR_UNSUPPORTED and a message naming the field.
 *   stream mode: every op with k > 1 keeps a ring of d(k - 1) rows of its own input (all sources concatenated), the head a
 *     ring of T_f - 1 rows of the last op's output, all zeros after create / reset (layers/stream.py:580-594); src_drop
 *     (StridedDrop) is the identity, the branches meet at the current frame (strided_drop.py:40-44).
 *   non_stream mode: the non-streaming model on the windows of `frames` rows ending at frames T, T + 1, ... <= L of every
 *     track; src_drop states the right alignment the kernel computes in.
 *   weights: Keras get_weights() order - per op kernel [k,1,Cin,F], gamma, beta, moving_mean, moving_variance [slots]
 *     (slots = bn_groups if > 1 else F); dense.kernel [T_f*C_last,1], dense.bias - folded once (eps 1e-3, channel c -> slot
 *     c mod g).
 *   mww_stream_get_state: the rows that can still influence an output, in op order - every op with k > 1: [d(k-1)][Cin] (an
 *     op fed by the spectrogram holds raw input frames), then the head [T_f-1][C_last]. */
int mww_stream_create_convnet(mww_ctx* ctx, const mww_convnet_desc* desc, int32_t mode, mww_stream** out);
/* The same graph stream (same vocabulary, refusals, weights and state layout, same handle type) on which the six int8 entry
 * points work: calibration on the float graph kernel, then the int8 graph kernel (csrc/tu_stream_graph_q8.hip) once
 * mww_stream_set_quantized has loaded parameters.  It is a creator of its own, and not a behaviour of the one above,
 * because the refusal of the int8 calls on a stream of mww_stream_create_convnet is pinned by the test-suite
 * (tests/test_inception_streaming_emulated.py): the old name keeps its behaviour, the feature arrives under a new one.
 *   tensors (mww_stream_num_tensors = n_ops + 2): 0 the input, 1 + i the output of op i (after folded BN/SSN + ReLU),
 *     n_ops + 1 the Dense logit.  mww_stream_calibrate_host: as below; the input range is taken from the fed frames, every
 *     other range over every position computed (a tile's halo only repeats real positions).
 *   mww_stream_set_quantized on such a stream:
 *     weights (int8): per op, output-major [Co][k][source 0: cn_0 rounded up to 4] ... [source n-1: cn rounded up to 4]
 *                     (padding entries 0; every op starts on a 4-byte boundary); then the Dense [T_f][C_last rounded up to 4]
 *     ints (int32):   per op: bias with the input zero point folded (b - zp_in * sum of the filter's weights over all taps
 *                     and channels) [cout], multiplier [cout], shift [cout]; the Dense's bias, multiplier, shift; then the
 *                     n_ops + 2 zero points.  All sources of an op share one scale and zero point (TFLite's CONCATENATION
 *                     constraint; microwakeword_amd/quantize_graph.py), which is what makes one folded bias exact.
 *     validation as for a MixedNet stream: sizes, zero points in [-128, 127], multipliers >= 0, shifts in [-31, 30].
 *   mww_stream_reset fills every ring with the zero point of the tensor it holds; mww_stream_get_state_q8 has the layout of
 *   mww_stream_get_state, one byte per value.  The uint8 output goes through the 256-entry table; probability
 *   (float)u8 * (float)(1/255) and the int8 logit (as float) land in the buffers mww_stream_read / _metrics read. */
int mww_stream_create_convnet_q8(mww_ctx* ctx, const mww_convnet_desc* desc, int32_t mode, mww_stream** out);
void mww_stream_destroy(mww_stream* s);
int64_t mww_stream_num_weights(const mww_stream* s);   /* floats of the Keras-order weight vector */
int64_t mww_stream_num_state(const mww_stream* s);     /* floats of the rings */
int mww_stream_set_weights(mww_stream* s, const float* keras_order, int64_t n);
int mww_stream_reset(mww_stream* s);                   /* rings back to zeros */
int mww_stream_get_state(mww_stream* s, float* host, int64_t n);   /* conv1 ring [R1][40], per MixConv [K-1][C], head [T_f-1][C] */
/* Runs the tracks (each a window of a resident store: pad_rows zero frames, then copy_rows store rows) in order as one call.
 * out_offsets [n_tracks + 1] receives the first output of every track; returns the number of outputs (or an error < 0).
 * The probabilities stay on the device (mww_stream_read, mww_stream_metrics). */
int64_t mww_stream_run(mww_stream* s, const mww_window* tracks, int64_t n_tracks, int64_t* out_offsets);
/* the same for one track of n_frames float32 rows in host memory */
int64_t mww_stream_run_host(mww_stream* s, const float* frames, int64_t n_frames);
int mww_stream_read(mww_stream* s, float* probs, float* logits, int64_t n);   /* either pointer may be NULL */
int mww_stream_set_probs(mww_stream* s, const float* probs, int64_t n);       /* host probabilities for mww_stream_metrics */
/* Detection metrics on the probabilities held (test.py:94-137,329-376): per track the moving average over `window`
 * probabilities (float32, summed in order), kind 0 (ambient): cooldown false-accept counts at each float64 cutoff (cooldown
 * starts at `cooldown`, is decremented with a floor at 0 before each value, a value > cutoff counts when it is 0 and resets
 * it) summed over the tracks into counts[n_cutoffs]; kind 1 (positive): score = max of the moving average of the
 * probabilities after the first `skip`.  ma_len[t]: moving-average values of track t (score is -inf when 0). */
int mww_stream_metrics(mww_stream* s, const int64_t* offsets, const int32_t* kind, int64_t n_tracks, int window, int skip,
                       int cooldown, const double* cutoffs, int n_cutoffs, uint64_t* counts, int64_t* ma_len, float* score);
/* WHERE the moving average crosses ONE cutoff (csrc/tu_stream_detect.hip), on the probabilities held - so on a
 * stream of any creator, float or int8.  Moving average, kinds, `skip` and the cooldown are those of mww_stream_metrics: a
 * track of n probabilities has m = n - window + 1 values avg_i (0 when n < window).
 *   kind 0 (ambient): index i is a detection iff (double)avg_i > cutoff and i >= next_ok, where next_ok starts at
 *     max(cooldown - 1, 0) and becomes i + max(cooldown, 1) after a detection (the closed form of test.py:119-135: cooldown
 *     starts at `cooldown`, is decremented with a floor at 0 before each value, a detection resets it).  Events
 *     (track, index, average) come ordered by track, then index; track_count[t] is the track's detections, complete whatever
 *     `capacity` is, and sums to what mww_stream_metrics counts at that cutoff; best_index[t] = -1, score[t] = 0.
 *   kind 1 (positive): after the first `skip` probabilities, score[t] = the maximum moving average (the bits of
 *     mww_stream_metrics) and best_index[t] = the smallest moving-average index, counted after the skip, that attains it
 *     (-1 and -inf when there is no value); track_count[t] = 0.
 * Returns the number of detections of the whole call, which may exceed `capacity`: the first `capacity` events are written
 * (out may be NULL when capacity is 0), or an error < 0.  Two calls on the same probabilities write the same bytes. */
typedef struct { int32_t track; int32_t reserved; int64_t index; float average; float reserved2; } mww_detection;
int64_t mww_stream_detections(mww_stream* s, const int64_t* offsets, const int32_t* kind, int64_t n_tracks, int window, int skip,
                              int cooldown, double cutoff, mww_detection* out, int64_t capacity, int64_t* track_count,
                              int64_t* best_index, float* score);
/* One mining round on the probabilities held (csrc/tu_stream_mine.hip): the hard negatives of the `tracks` that
 * were run (their `offsets` as mww_stream_run returned them), every track ambient (kind 0), selected and cut into clips on the
 * device.  Byte for byte the chain it replaces:
 *   detections  those of mww_stream_detections at `window`, `cooldown`, `cutoff` (skip does not apply to ambient tracks);
 *   selection   max_new < 0 keeps every event, else the max_new highest moving averages (compared as floats: -0 == +0), ties
 *               to the earlier event in (track, index) order - a stable descending sort - returned in (track, index) order;
 *   clips       streaming.detection_clips: output n = index + window - 1 was computed from the track rows ending at
 *               e = (n + 1) * stride (stream mode) or frames + n * stride (non_stream mode; frames, stride and mode are the
 *               stream's own); the clip is rows [e - frames - before, e + after) minus the track's pad_rows, clipped to
 *               [0, copy_rows), as (store, 0, rows, 0, src_elem + 40 * first row).  A selected event without a row is dropped
 *               AFTER the selection, so fewer than max_new clips may remain.
 * clips / events [capacity] receive the first `capacity` kept clips and their events in (track, index) order (both may be NULL
 * when capacity is 0); *n_detections the detections before the selection; track_count [n_tracks] each track's detections.
 * Returns the number of clips kept, which may exceed `capacity`, or an error < 0.  The host reads back at most
 * min(max_new, capacity) clips and events and the counts, never the event list.  Two calls on the same probabilities write the
 * same bytes. */
int64_t mww_stream_mine(mww_stream* s, const mww_window* tracks, const int64_t* offsets, int64_t n_tracks, int window, int cooldown,
                        double cutoff, int before, int after, int64_t max_new, mww_window* clips, mww_detection* events,
                        int64_t capacity, int64_t* n_detections, int64_t* track_count);
/* The grid a deployment is chosen from (csrc/tu_stream_oppoints.hip): row k of counts [n_windows][n_cutoffs],
 * ma_len [n_windows][n_tracks] and score [n_windows][n_tracks] is exactly what mww_stream_metrics returns for window = windows[k]
 * with the same other arguments - the same integers, the same score bits - with the semantics its comment states (moving
 * average, comparison, cooldown, `skip`, empty tracks).  `windows` may be unsorted and may repeat; each lies in
 * 1..MWW_OP_MAX_WINDOW, n_windows in 1..MWW_OP_MAX_WINDOWS, n_cutoffs in 1..128.  On the probabilities held, so on a stream
 * of any creator, float or int8.  Two calls on the same probabilities write the same bytes. */
#define MWW_OP_MAX_WINDOWS 32
#define MWW_OP_MAX_WINDOW 256
int mww_stream_operating_points(mww_stream* s, const int64_t* offsets, const int32_t* kind, int64_t n_tracks, const int32_t* windows,
                                int n_windows, int skip, int cooldown, const double* cutoffs, int n_cutoffs, uint64_t* counts,
                                int64_t* ma_len, float* score);
/* The same grid summarised on the device (csrc/tu_stream_oppoints.hip): what a choice of operating point reads,
 * whatever the number of tracks.  With score[k][t] and ma_len[k][t] the values mww_stream_operating_points returns (the skip
 * applies to kind 1; an empty track has score -inf and length 0) - they stay on the device -:
 *   counts [n_windows][n_cutoffs]        exactly the counts of mww_stream_operating_points (the kind-0 tracks);
 *   accepts [n_windows][n_cutoffs]       the kind-1 tracks with (double)score[k][t] > cutoffs[c], strict: a score equal to the
 *                                        cutoff is not accepted, -inf never; frr = 1 - accepts / n_kind[1] on the host;
 *   hours [n_windows]                    the float64 sum over the kind-0 tracks, in track order, of
 *                                        ((double)(ma_len[k][t] * stride) * step_s) / 3600.0: product, division and add are
 *                                        separate IEEE operations (streaming.track_hours, bit for bit);
 *   short_tracks [n_windows][2]          the kind-0 / kind-1 tracks with ma_len[k][t] == 0: a window is usable when n_kind[0] > 0
 *                                        and both are 0;
 *   n_kind [2]                           the kind-0 / kind-1 tracks.
 * A kind-1 track takes no part in the per-cutoff walk and has no per-track count row; its score is compared with the cutoffs in
 * an integer reduction of fixed order.  The host reads back n_windows * n_cutoffs * 16 + n_windows * 24 + 16 bytes.  Arguments
 * and limits are those of mww_stream_operating_points; in addition stride >= 1 and step_s > 0.  On the probabilities held, so on
 * a stream of any creator, float or int8.  Two calls on the same probabilities write the same bytes. */
int mww_stream_operating_summary(mww_stream* s, const int64_t* offsets, const int32_t* kind, int64_t n_tracks, const int32_t* windows,
                                 int n_windows, int skip, int cooldown, const double* cutoffs, int n_cutoffs, int stride, double step_s,
                                 uint64_t* counts, uint64_t* accepts, double* hours, int64_t* short_tracks, int64_t* n_kind);
/* The grid of mww_stream_operating_summary resampled on the device (csrc/tu_stream_bootstrap.hip): `replicates`
 * bootstrap replicates over the evaluation units, one record each read back - replicates * sizeof(mww_boot_record) bytes,
 * whatever the tracks, windows and cutoffs.  Inputs and limits are those of mww_stream_operating_summary; here `cutoffs` must
 * ascend strictly (MWW_ERR_INVALID otherwise: the selection rule assumes it, and a positive is then stored as one level).
 * Everything below is integer arithmetic or single IEEE float64 operations (no contraction): streaming.operating_bootstrap_host
 * restates it, byte for byte.
 *   units      a positive unit is a kind-1 track (n_pos of them).  An ambient unit is a block of a kind-0 track: with block = 0
 *              every kind-0 track is one block, an empty one too; with block = L > 0, a positive multiple of
 *              MWW_BOOT_BLOCK_UNIT, a track of n probabilities has ceil(n / L) blocks, whatever the window, and at window k
 *              block b owns the moving-average indices [b L, min((b + 1) L, m_k)), possibly none.  A block's count at (k, c)
 *              is the number of the track's detections whose index it owns - detections of the whole-track cooldown walk of
 *              mww_stream_metrics, so the cooldown carries across block borders and a track's blocks sum to its count -, its
 *              length at k the size of its index range.  NB is the number of blocks, in (track, block) order.
 *   draws      draw(seed, kind, r, i, n): ctr = kind << 56 | r << 32 | i; z = seed + ctr * 0x9E3779B97F4A7C15 (mod 2^64);
 *              z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31 (the splitmix64
 *              finaliser); the result is ((z >> 32) * n) >> 32: a multiply-shift without rejection, its bias below n / 2^32.
 *              Replicate r draws the NB blocks draw(seed, 0, r, i, NB), i < NB, and the n_pos positives draw(seed, 1, r, i,
 *              n_pos), i < n_pos; one set of draws serves all windows.
 *   grid       counts_r[k][c] = the sum of the drawn blocks' counts, slices_r[k] = the sum of their lengths (int64),
 *              accepts_r[k][c] = the drawn positives with (double)score[k][t] > cutoffs[c] (strict; -inf never);
 *              hours_r[k] = ((double)(slices_r[k] * stride) * step_s) / 3600.0, faph_r = (double)counts_r / hours_r,
 *              frr_r = 1 - (double)accepts_r / n_pos.  A window is usable in a replicate when it is usable on the full data
 *              (a kind-0 and a kind-1 track exist, none is without a moving-average value) and slices_r[k] > 0.
 *   record     sel_row, sel_cutoff: streaming.select_operating_points(faph_r, frr_r, usable_r, target_faph, windows) - per
 *              usable window the smallest cutoff with faph_r <= target_faph there and at every larger cutoff, then the window
 *              of the smallest (frr_r, faph_r, window, row) -, (-1, -1) when no window meets the target; sel_counts,
 *              sel_slices, sel_accepts: counts_r, slices_r, accepts_r there (0 without a point).  fixed_*: the same three at
 *              (fixed_row, fixed_cutoff), a point of the grid, or 0 with fixed_row = fixed_cutoff = -1.
 * The re-selected point gives the uncertainty of the metric a selection rests on, the fixed point that of a cutoff that ships.
 * max_scratch_bytes caps the device scratch of the block tables, 4 W NB C + 8 W NB + W n_pos bytes (0: 256 MiB); beyond it the
 * call is MWW_ERR_UNSUPPORTED and asks for a larger block.  A refused call leaves the probabilities held as they are.  On the
 * probabilities held, so on a stream of any creator, float or int8.  Two calls on the same probabilities write the same bytes. */
#define MWW_BOOT_BLOCK_UNIT 1024
#define MWW_BOOT_MAX_REPLICATES 65536
typedef struct {
  int32_t sel_row, sel_cutoff;
  uint64_t sel_counts; int64_t sel_slices; uint64_t sel_accepts;
  uint64_t fixed_counts; int64_t fixed_slices; uint64_t fixed_accepts;
} mww_boot_record;
int mww_stream_operating_bootstrap(mww_stream* s, const int64_t* offsets, const int32_t* kind, int64_t n_tracks, const int32_t* windows,
                                   int n_windows, int skip, int cooldown, const double* cutoffs, int n_cutoffs, int stride, double step_s,
                                   int replicates, uint64_t seed, int64_t block, double target_faph, int fixed_row, int fixed_cutoff,
                                   int64_t max_scratch_bytes, mww_boot_record* records);

/* ---- int8 quantized streaming model (the reference's --test_tflite_streaming_quantized; microwakeword_amd/quantize.py
 * derives the parameters, INTEGRATION.md states the contract).
 * Calibration: tensors, in order, are the input, conv1 (after ReLU), every layer of the plan (a MixConv layer's output with
 * its groups concatenated, a 1x1 layer's output after folded BN + ReLU), the Dense logit: mww_stream_num_tensors of them.
 * mww_stream_calibrate_host runs the float streaming model (stream mode, from the state it has, which it carries on) over
 * n_frames host rows and writes ranges[n_tensors][2] = min, max over every position computed; the probabilities
 * are those of mww_stream_run_host on the same frames, bit for bit. */
int mww_stream_num_tensors(const mww_stream* s);
int mww_stream_calibrate_host(mww_stream* s, const float* frames, int64_t n_frames, float* ranges);
/* The same calibration over windows of resident stores (csrc/tu_stream_calibrate.hip): mww_stream_run over
 * `tracks` with the <REC> form of the float kernel, from the float state the stream has, which it carries on - whether or not
 * mww_stream_set_quantized has loaded parameters (the float weights stay; the ranges are the same).  Probabilities, logits,
 * out_offsets and the float rings are those of mww_stream_run on the same tracks on a float stream, bit for bit.
 *   tracks   every track's pad_rows + copy_rows must be a multiple of the stream's stride (MWW_ERR_INVALID naming the track
 *            otherwise): then no frame is dropped between tracks and the call is one concatenated stream, which is what a
 *            converter's calibrator sees.  n_tracks == 0 is MWW_ERR_INVALID.
 *   ranges   [n_tensors][2].  ranges[0], the input tensor: min / max over every frame fed, the pad_rows zero frames included, a
 *            u16 store value scaled by 0.0390625 as the kernels read it.  ranges[t], t >= 1: the fold, in workgroup order, of the
 *            launch's per-workgroup partial rows.  Both reductions run on the device (LDS folds of fixed order, no atomics);
 *            the host reads n_tensors * 8 bytes and uploads nothing but the call's tables.
 * `ranges` equals what mww_stream_calibrate_host returns from a stream in the same state on the host rows of the same windows
 * concatenated (zero rows for the padding).  A stream without the int8 entry points answers as mww_stream_calibrate_host does.
 * Returns the number of outputs, or an error < 0. */
int64_t mww_stream_calibrate(mww_stream* s, const mww_window* tracks, int64_t n_tracks, int64_t* out_offsets, float* ranges);
/* Loads int8 parameters; from then on mww_stream_run / _run_host run the int8 kernel (the float weights stay for
 * calibration) and mww_stream_reset fills every ring with its tensor's zero point.  The plan's ops, in order: conv1, every
 * layer (MixConv: depthwise taps of all groups fused to K = max kernel taps, right-aligned; 1x1), the Dense.
 *   weights (int8): conv1 [C1][k1*40]; MixConv [K][C]; 1x1 [Co][Ci rounded up to 4]; Dense [T_f][C_last rounded up to 4]
 *                   (padding entries 0)
 *   ints (int32):   per op: bias with the input zero point folded (b - zp_in * sum of the channel's weights) [cout],
 *                   multiplier [cout], shift [cout] (TFLite QuantizeMultiplier); then the n_tensors zero points
 *   input_scale:    the input tensor's scale (its zero point is the first of the zero points)
 *   lut (uint8):    [256] logit q + 128 -> the uint8 output; probability = (float)u8 * (float)(1/255)
 * On a stream of mww_stream_create_mixednet_q8 whose plan has a residual block or a pooled head (a plain plan keeps every
 * offset above):
 *   tensors:  input, conv1; per block: its residual r (1x1 + folded BN of the block input, linear) when it has one, in front
 *             of its repeats; per repeat: the MixConv output (when max(ks) > 1), the 1x1 output (with a residual: linear,
 *             BEFORE the add), the ADD output (after the fused ReLU; only with a residual); the Dense logit.
 *   ops:      conv1; per block the residual 1x1 (when it has one), per repeat MixConv and 1x1; the Dense.
 *   weights:  the residual 1x1 and a residual block's 1x1 are [Co][Ci rounded up to 4] like any 1x1; a pooled Dense is
 *             [1][C_last rounded up to 4] (it reads the C pooled values).
 *   ints:     per op bias / multiplier / shift [cout] as above; a residual block's 1x1 is followed by the six integers of
 *             its ADD: M1, sh1 (the 1x1 output), M2, sh2 (r), Mo, sho (TFLite int8 Add, left_shift 20: QuantizeMultiplier
 *             of s1 / (2 max(s1, s2)), s2 / (2 max(s1, s2)), 2 max(s1, s2) / (2^20 s_out); multipliers >= 0, shifts in
 *             [-31, 0]); then the n_tensors zero points in the tensor order above.
 *   rings:    unchanged; the MixConv of a repeat >= 1 of a residual block holds the previous ADD output, the head ring the
 *             final map (the ADD output when the last block has a residual); reset fills each with that tensor's zero point.
 *   pooling:  the pooled value shares the final map's scale and zero point; average: acc = sum of the T_f int8 values,
 *             (acc > 0 ? acc + T_f / 2 : acc - T_f / 2) / T_f (C division), clamped; max: the int8 maximum. */
int mww_stream_set_quantized(mww_stream* s, const int8_t* weights, int64_t n_weights, const int32_t* ints, int64_t n_ints,
                             float input_scale, const uint8_t* lut);
int64_t mww_stream_q8_sizes(const mww_stream* s, int64_t* n_ints);   /* int8 weights expected (n_ints: int32 entries) */
/* uint8 outputs of the last int8 run; int8 rings (the layout of mww_stream_get_state, one byte per value) */
int mww_stream_read_q8(mww_stream* s, uint8_t* out, int64_t n);
int mww_stream_get_state_q8(mww_stream* s, int8_t* host, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* MWW_H */
