/*
 * alq.h - C ABI of the MI355X-native active-learning query-scoring library (libalq.so).
 *
 * The reference (jsourati/nn-active-learning) has no FFI: its device boundary is
 * `sess.run(...)` on a TensorFlow-1.x graph.  Each entry point below names the reference
 * call site(s) whose device work it replaces (file:line under /root/reference).
 *
 * Conventions
 *   - plain C, no torch / C++ types in any signature;
 *   - every function returns an int status: 0 = ok, negative = error
 *     (alq_last_error() gives the text); nothing throws, nothing exits;
 *   - pointers named `d_*` are DEVICE pointers owned by the caller (e.g. torch-ROCm
 *     tensors); pointers named `h_*` are HOST pointers; the library never frees caller memory;
 *   - all work is enqueued on the stream given to alq_ctx_create (a hipStream_t passed as
 *     void*; NULL = the null stream) and is stream-ordered; the calls do not synchronise
 *     unless documented.  A context also owns one private side stream: alq_fisher runs the
 *     per-layer statistics kernels there, forked from and joined back into the caller's stream
 *     with events inside the call, so every result is ordered on the caller's stream as if the
 *     whole call had run on it (ALQ_NO_SIDE_STREAM=1 at context creation: one stream only);
 *   - tensors are channels-last fp32: patches [N, D, H, W, C] (D = 1 for the 2-D nets,
 *     i.e. the reference's [N, H, W, C] placeholder, NN.py:1338-1344).
 */
#ifndef ALQ_H
#define ALQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct alq_ctx alq_ctx;
typedef struct alq_model alq_model;

enum { ALQ_OK = 0, ALQ_EINVAL = -1, ALQ_EHIP = -2, ALQ_ENOMEM = -3, ALQ_EUNSUPPORTED = -4 };

enum { ALQ_CONV = 0, ALQ_CONVT = 1, ALQ_POOL = 2, ALQ_FC = 3 };

/* One layer of the reference's layer dicts (NN.py:96-110; NN_extended.py:103-124). */
typedef struct {
    int32_t type;      /* ALQ_CONV / ALQ_CONVT / ALQ_POOL / ALQ_FC                               */
    int32_t cout;      /* output channels (conv, conv_transpose) or units (fc); unused for pool  */
    int32_t k[3];      /* kernel (conv / conv_transpose) or window (pool), order D,H,W; 1 = n/a  */
    int32_t s[3];      /* strides, order D,H,W                                                   */
    int32_t relu;      /* 1: ReLU after the main op (NN.py:290,326-327; 'A' in NN_extended.py:352-355) */
    int32_t skip_src;  /* index of the earlier layer whose OUTPUT is concatenated IN FRONT of this
                          layer's input ('con' skip, NN_extended.py:1207-1214), or -1            */
} alq_layer_t;

const char *alq_last_error(void);
int alq_version(void);

/* ---- context ---------------------------------------------------------------------------- */
/* Replaces: tf.Session creation (PW_AL.py:363-377).  `stream` is a hipStream_t or NULL.       */
int alq_ctx_create(int device, void *stream, alq_ctx **out);
int alq_ctx_destroy(alq_ctx *ctx);
/* Moves the context to another stream; the new stream first waits (event) for everything the library enqueued on the old
 * one, so back-to-back calls on two streams need no host synchronisation.                                           */
int alq_ctx_set_stream(alq_ctx *ctx, void *stream);
/* on = 0: the per-layer statistics kernels of later alq_fisher calls stay on the caller's stream instead of the context's side
 * stream (on = 1, the default, restores it).  For a caller that overlaps WHOLE passes on two contexts (device.DeviceModel's two
 * scoring pipelines): the other pipeline's launches already fill the gaps, and four streams competing cost 1.2 % (round 6).
 * Results do not depend on it (same kernels, same order per context).                                                      */
int alq_ctx_use_side_stream(alq_ctx *ctx, int on);
int alq_ctx_synchronize(alq_ctx *ctx);

/* ---- model ------------------------------------------------------------------------------ */
/* Replaces: graph construction NN.CNN.__init__ (NN.py:147-188) / NN_extended.CNN.__init__
 * (NN_extended.py:187-295) + get_gradients (NN.py:621-645).  in_dims = {D, H, W, C}.
 * max_batch = largest N any later call will pass (activation workspace is sized for it).     */
int alq_model_create(alq_ctx *ctx, const alq_layer_t *layers, int n_layers,
                     const int32_t in_dims[4], int max_batch, alq_model **out);
int alq_model_destroy(alq_model *m);
/* Patches per device pass the model's workspace holds: min(max_batch asked for, what the engines' unsigned 32-bit tensor
 * offsets allow - every allocation below 2^30 floats; NET-C at 32^3: 2047).  A larger batch is walked in passes of this
 * size by the host (the reference feeds `ntb` patches per sess.run, PW_NN.py:447-451: the split never changes a result). */
int alq_model_max_batch(const alq_model *m);
/* Fully-convolutional ("dense") models.  alq_model_create also takes a last layer of type ALQ_CONV when k = s = {1,1,1},
 * relu = 0, skip_src < 0, 2 <= cout <= 8, the layer feeds no concat, and its input is a dense tensor of C channels, C % 4 == 0,
 * C <= 64 (any other non-fc last layer: ALQ_EUNSUPPORTED, the message names the condition).  Every voxel of the head's output
 * is then a sample: with V = alq_model_out_voxels (1 for an fc-head model; voxel index v in the activation's memory order)
 *   alq_forward / alq_forward_dropout   d_post [c, N V] class-major planes (sample n V + v), d_pred int64 [N V];
 *   alq_param_grads_loss                d_labels int32 [N V] (outside [0, c): unlabelled voxel), loss->d_sample_w [N V],
 *                                       d_targets / d_old_logits / d_post [c, N V]; statistics with voxels as samples;
 *   alq_loss_stats                      model-free: call it with N V samples.
 * The head keeps its weights as plain fp32 [Ci][c] + [c] - the bytes of the TF filter [1, (1,) 1, Ci, c] both weight setters
 * take.  alq_model_max_batch also keeps N V below 2^31.  alq_fisher*, alq_forward_rows, alq_param_grads, alq_grad_sqnorms,
 * alq_class_layer_sums, alq_diag_fisher and alq_hess_vecp return ALQ_EUNSUPPORTED for such a model before any launch.       */
int alq_model_out_voxels(const alq_model *m);
/* The head's kernels on their own (csrc/dense.hip), model-free: d_x [R, Ci] (16-byte aligned, Ci % 4 == 0, Ci <= 64), d_W [Ci, c],
 * d_b [c], 2 <= c <= 8 -> d_post [c, R], d_pred int64 [R] or NULL; backward: d_delta [R, c] -> d_dx [R, Ci] (NULL: not wanted) and
 * d_dW_db = [dW (Ci c), db (c)], through d_work of alq_dense_head_work_bytes(Ci, c) bytes.  Bit-identical from run to run.           */
size_t alq_dense_head_work_bytes(int Ci, int c);
int alq_dense_head_fwd(alq_ctx *ctx, const float *d_x, int64_t R, int Ci, int c, const float *d_W, const float *d_b, float *d_post,
                       int64_t *d_pred);
int alq_dense_head_bwd(alq_ctx *ctx, const float *d_delta, const float *d_x, int64_t R, int Ci, int c, const float *d_W, float *d_dx,
                       void *d_work, float *d_dW_db);
/* The forward kernel for a head with an aleatoric-uncertainty channel (AU_4U, NN_extended.py:265-288): d_W [Ci, c + 1], d_b [c + 1],
 * 2 <= c <= 7.  d_post [c, R] = softmax over the first c channels and d_pred (or NULL) their first maximum - the bits
 * alq_dense_head_fwd writes for W[:, :c], b[:c] (every channel keeps its own chain of fused multiply-adds) -, d_au [R] =
 * max(z_c, 0), the per-voxel log-variance, d_logits [R, c + 1] or NULL.  ALQ_EINVAL: a null pointer (d_au included);
 * ALQ_EUNSUPPORTED: Ci or c outside the limits.                                                                                      */
int alq_dense_head_fwd_au(alq_ctx *ctx, const float *d_x, int64_t R, int Ci, int c, const float *d_W, const float *d_b, float *d_post,
                          int64_t *d_pred, float *d_au, float *d_logits);
/* The launch arithmetic of alq_dense_head_bwd over R rows of Ci channels, as the launch itself computes it (no device call): the
 * workgroups (at most 2048), the rows each of them owns, the rows one sweep of a workgroup covers (256 / (Ci / 4)) and the rows a
 * lane sums in fp32 before they go into its fp64 sums.  A workgroup owning more than flush_rows * rows_per_sweep rows folds more
 * than once.  For tests: a case asserts from these that it is in the regime it names.  ALQ_EINVAL: a null pointer or R < 1;
 * ALQ_EUNSUPPORTED: Ci as for the launch.                                                                                         */
int alq_dense_head_bwd_geometry(int64_t R, int Ci, int *blocks, int64_t *rows_per_block, int *rows_per_sweep, int *flush_rows);
/* Number of parameterised layers L ( = len(grad_posts['1'])/2, PW_NNAL.py:751 ).             */
int alq_model_num_param_layers(const alq_model *m);
/* W/b element counts of parameterised layer t (creation order), i.e. prod(W.shape), len(b).  */
int alq_model_param_sizes(const alq_model *m, int t, int64_t *w_elems, int64_t *b_elems);
/* Length of the feature vector of layer `layer_idx`'s output (feature_layer, NN.py:172-175). */
int alq_model_layer_out_elems(const alq_model *m, int layer_idx, int64_t *elems);
/* Replaces: CNN.load_weights / perform_assign_ops (NN.py:396-419, :462-519).  HOST pointers,
 * TF layouts: conv [k...,Ci,Co], conv_transpose [k...,Co,Ci], fc [out,in] with `in` in the
 * reference's flatten order (full axis reversal, NN.py:296-301); bias [Co] / [out,1].
 * Synchronises the stream before returning (the host buffers may be reused at once).         */
int alq_model_set_weights(alq_model *m, int t, const float *h_W, const float *h_b);
/* Same contract as alq_model_set_weights, but d_W / d_b are DEVICE pointers (TF layouts, fp32, any 4-byte alignment), e.g. slices
 * of the flat parameter vector that alq_sgd_step / alq_adam_step just updated: the model ends up in the state the host call
 * would have left with the same values, and every entry point returns the same bits.  Stream-ordered on the context's stream:
 * the buffers must be ready there (a producer on another stream: order it with an event first).
 * A wide fully connected layer - forward and backward Gemm both on the streaming GEMM of csrc/fcgemm.hip: inputs and units
 * multiples of 64, both >= 256 (alq_model_layer_packs_on_device) - is packed by HIP kernels (csrc/wpack.hip): flatten
 * permutation, bf16 triples and fp16 pairs of both Gemm orientations, the layer's L1 bound.  No weight element of such a layer
 * crosses to the host; the call reads back 16 bytes (at most 64 by contract) for the host-side scalars - the bound and the
 * fp16 scale exponent - and synchronises the stream for that.  Its raw fp32 weights stay resident; the forms of the engines
 * that only the debug knobs select behind the streaming GEMM are packed from them on the host when a call first needs them.
 * Any other layer (conv / conv_transpose engines, the two-class head, narrow fc layers) is not an error: its slice is copied to
 * the host and goes through alq_model_set_weights.  Works before any host call (first-call allocations).
 * ALQ_EINVAL: null pointer, no parameterised layer t.                                                                     */
int alq_model_set_weights_device(alq_model *m, int t, const float *d_W, const float *d_b);
/* 1 when alq_model_set_weights_device packs parameterised layer t with the device kernels, 0 when it takes the host packers;
 * negative error code for a bad t.                                                                                        */
int alq_model_layer_packs_on_device(const alq_model *m, int t);
/* The launch arithmetic of the streaming GEMM (csrc/fcgemm.hip) for a contraction of K inputs into N features over M rows, as
 * the launches themselves compute it (no device call): out[6] = {wide (0 / 1: fcgemm_build_plan takes the shape - K a multiple of
 * 32, N of 64, both >= 256), features per workgroup tile of the fp16-pair launches (64 / 128), tall wave tiles (0 / 1), grid.x,
 * grid.y, k-steps}.  Reads ALQ_FC_BN64 / ALQ_FC_SQUARE as plan building does.  The bf16-triple launch of a wide shape always
 * takes 64-feature tiles (grid.x = N / 64) over the same rows and k-steps.  A shape the plan declines: out = zeros, no error.
 * A layer's backward Gemm is the same call with K and N swapped.  For tests: a case asserts from these that it is in the regime
 * it names.  ALQ_EINVAL: null out or a non-positive size.                                                                   */
int alq_fcgemm_geometry(int K, int N, int M, int *out);

/* ---- patch gather + normalisation ------------------------------------------------------- */
/* Replaces: patch_utils.get_patches (patch_utils.py:1087-1173) + the normalisation loops of
 * PW_NN.batch_eval (PW_NN.py:503-506) / PW_NNAL.CNN_query (PW_NNAL.py:125-129) [quirk = 1:
 * channel j < m is normalised with stats[j]] or of patch_utils.get_patches_multimg
 * (patch_utils.py:1203-1207) [quirk = 0: depth slab j*d3..(j+1)*d3 with stats[j]].
 * d_vols: m device pointers (host array of device pointers) to zero-padded volumes, C order,
 * element type double (vol_is_f64 = 1) or float; pad_dims = padded shape; d_inds: int64
 * raveled indices in UN-padded coordinates; h_stats: m pairs (mu, sigma), double.
 * quirk = 2: no normalisation (plain get_patches).  d_out: [n, d1, d2, m*d3], float
 * (out_is_f64 = 0) or double (out_is_f64 = 1, bit-identical to the reference's float64
 * patches).  Arithmetic is fp64, rounded once to fp32 for the float output, like the
 * reference's float64 patches fed to a float32 placeholder.                                  */
int alq_gather_normalize(alq_ctx *ctx, const void *const *d_vols, int m, int vol_is_f64,
                         const int64_t pad_dims[3], const int64_t *d_inds, int64_t n,
                         const int32_t patch_shape[3], const double *h_stats, int quirk,
                         int out_is_f64, void *d_out);

/* ---- forward ---------------------------------------------------------------------------- */
/* Replaces: sess.run(model.posteriors / prediction / feature_layer) in PW_NN.batch_eval
 * (PW_NN.py:522-524).  d_x: [N, D,H,W,C]; d_post: [2... c, N] row-major like the reference's
 * [c, N] posteriors (NN.py:184-188); d_pred: int64 [N] or NULL; d_feat: [N, F] of layer
 * feature_layer_idx (or NULL / -1).  N <= max_batch.                                         */
int alq_forward(alq_model *m, const float *d_x, int N, float *d_post, int64_t *d_pred,
                float *d_feat, int feature_layer_idx);

/* Same, on rows of a resident pool: patch i of the batch is d_pool[d_rows[i]] (d_pool: [n_pool, D,H,W,C] fp32,
 * d_rows: int64 [N] device).  Replaces the `inds[batches[j]]` indirection of PW_NN.batch_eval (PW_NN.py:447-451,
 * :498-501) for pools that live in HBM: the caller passes positions instead of gathering a copy of the patches. */
int alq_forward_rows(alq_model *m, const float *d_pool, const int64_t *d_rows, int N, float *d_post,
                     int64_t *d_pred, float *d_feat, int feature_layer_idx);

/* ---- uncertainty scores ----------------------------------------------------------------- */
/* Replaces: np.abs(posts - .5) (PW_NNAL.py:64,109,728) and NNAL_tools.compute_entropy
 * (NNAL_tools.py:71-85).  d_p1: float [n] (row 1 of the posteriors); d_absdev: double [n]
 * = |double(p1) - 0.5| (exact); d_H: float [n] Shannon entropy of (1-p1, p1) with the
 * reference's +10e-8 guard on exact zeros, or NULL.                                          */
int alq_score_entropy(alq_ctx *ctx, const float *d_p1, int64_t n, double *d_absdev, float *d_H);

/* Replaces: np.argsort(np.abs(posts - .5))[:B] (PW_NNAL.py:64,109-110,671-681,730).
 * Ascending keys, ties -> lower index first (the reference's tie order is unspecified).
 * Keys compare in numeric order for either sign (a NaN with the sign bit clear after +inf, a NaN with the sign bit SET before
 * -inf: the order is that of sign and magnitude bits, so such a key is picked FIRST - keep it out of the keys); -0.0 sorts
 * immediately before +0.0, so a caller whose keys may be zero of either sign writes them as 0.0 - x, which is never -0.0.
 * d_keys is only read; B = 0 touches neither d_out_idx nor d_work; B > n, B < 0 and n < 0 are ALQ_EINVAL.
 * d_out_idx: int64 [B].  d_work: device scratch of alq_topk_work_bytes(n) bytes.             */
size_t alq_topk_work_bytes(int64_t n);
int alq_topk_uncertain(alq_ctx *ctx, const double *d_keys, int64_t n, int64_t B,
                       int64_t *d_out_idx, void *d_work);

/* Replaces: the committee loop of the `ensemble` and `QBC-JS` queries (PW_NNAL.py:453-545), one member per call.
 * d_p1: float [n] class-1 posteriors of member `member` (0-based; members in order); d_mean_p: double [n] running mean
 * posterior av = (p + i*av) / (i+1); mode ALQ_COMMITTEE_QBC_JS also keeps d_mean_h: double [n] running mean entropy
 * avH = (ent(p) + i*avH) / (i+1), ent(x) = -x*log(x) - (1-x)*log(1-x) with an exact 0 in x or in 1-x lifted to 1e-6
 * first (d_mean_h may be NULL for ALQ_COMMITTEE_ENSEMBLE).  At member 0 the buffers are written, not read.
 * d_keys (optional, typically at the last member): double [n] keys for alq_topk_uncertain, ensemble |av - .5|,
 * QBC-JS 0.0 - (ent(av) - avH) (never -0.0).  Every float64 operation is NumPy's in the reference's order (no
 * contraction): av and the ensemble keys are bit-exact; entropies differ from NumPy's only by the device log.       */
#define ALQ_COMMITTEE_ENSEMBLE 0
#define ALQ_COMMITTEE_QBC_JS 1
int alq_committee_update(alq_ctx *ctx, const float *d_p1, int64_t n, int member, int mode, double *d_mean_p,
                         double *d_mean_h, double *d_keys);

/* Replaces: PW_analyze_results.get_preds_stats (PW_analyze_results.py:234-258) on the predictions of one chunk of evaluated
 * voxels - what Experiment_MultiImg.test_eval (PW_AL.py:653-668), full_model_eval (PW_analyze_results.py:649-651) and
 * grid_based_F1 (:794-795) call it on after copying every PW_NN.batch_eval(..., 'prediction') vector to the host - and the
 * scatter `preds[:, :, ind] = slice_evals` / np.uint8(preds) of full_model_eval (:613-625, :663-665).
 * d_pred: int64 [n] as alq_forward writes it; d_inds: int64 [n] raveled UN-padded voxel indices (those of
 * alq_gather_normalize) into d_mask, the subject's un-padded mask volume of mask_elems elements, float or double
 * (mask_is_f64 = 1), resident on the device; it may hold NaN.  The label of sample i is mask[d_inds[i]]; d_inds NULL: d_mask
 * is already the label vector (n <= mask_elems), as with the labels of gen_multimg_inds (PW_AL.py:921-975).
 * d_counts: int64 [6] = P, N, TP, FP, TN, FN; the call ADDS to them (the caller zeroes them; they stay on the device over all
 * chunks and subjects): P += mask > 0, N += mask == 0, TP += pred > 0 && mask > 0, FP += pred > 0 && mask == 0,
 * TN += pred == 0 && mask == 0, FN += pred == 0 && mask > 0 - a NaN or a negative label counts nowhere, as in NumPy.
 * d_seg (optional): uint8 un-padded volume, d_seg[d_inds[i]] = pred[i] (d_seg[i] without indices; distinct indices);
 * other bytes are left alone.  Integer sums: exact and bit-identical whatever the chunking, the grid or the launch order.
 * An index outside [0, mask_elems) is skipped on the device (nothing read, written or counted for it) and the call returns
 * ALQ_EINVAL: with d_inds the call therefore synchronises the stream (one 4-byte flag read); without, it does not.
 * n = 0: nothing is done.                                                                                                   */
int alq_eval_counts(alq_ctx *ctx, const int64_t *d_pred, const int64_t *d_inds, int64_t n, const void *d_mask,
                    int mask_is_f64, int64_t mask_elems, int64_t *d_counts, uint8_t *d_seg);

/* Multi-class confusion counts over resident label maps (csrc/confusion.hip).
 * Replaces: the two np.argmax, the concatenation and the NumPy counting of eval_utils.eval_metrics (eval_utils.py:55-98) and the
 * per-partition np.sum(preds*labels) of eval_utils.eval_full_segs_explicit_partitions / _label_percentage (:240-363).
 * d_pred, d_lab: n ids each, uint8, int32 or int64 (the ALQ_IDS_* of their own).  For element i, with j = first + i and
 * g = (j / inner) % groups: t = lab[i], replaced by `fill` when t lies outside [0, C) and 0 <= fill < C; the element is
 * skipped when t (after that) or p = pred[i] lies outside [0, C); otherwise d_counts[g][t][p] += 1.
 * d_counts: int64 [groups, C, C]; the call ADDS (the caller zeroes).  d_skipped (optional): int64 [1], += skipped elements.
 *   whole batch: inner = n, groups = 1;  per sample of [b, h, w]: inner = h w, groups = b;
 *   per axial slice of an [H, W, Z] volume in C order: inner = 1, groups = Z;  per slice of a packed [Z, H, W]: inner = H W,
 *   groups = Z.  `first` makes a chunked sequence of calls equal to one call.
 * 1 <= C <= 16, inner >= 1, groups >= 1, first >= 0, n >= 0 (n = 0: nothing is done).  Integer sums: exact and bit-identical
 * whatever the chunking, the grid or the launch order.  groups C^2 cells beyond the kernel's histogram: one launch per window of
 * alq_confusion_window(C) groups (0 for a C out of range).  Stream-ordered, no synchronisation.  ALQ_EINVAL before any launch:
 * a null pointer (d_skipped aside), an unknown type, a bound broken, a pointer not aligned to its element.                    */
enum { ALQ_IDS_U8 = 0, ALQ_IDS_I32 = 1, ALQ_IDS_I64 = 2 };
int alq_confusion_counts(alq_ctx *ctx, const void *d_pred, int pred_type, const void *d_lab, int lab_type, int64_t n, int64_t first,
                         int64_t inner, int64_t groups, int C, int fill, int64_t *d_counts, int64_t *d_skipped);
int alq_confusion_window(int C);

/* Slice queries of a fully-convolutional model (csrc/sliceq.hip).  No reference counterpart: the reference stops at the
 * (c, h, w, z) uncertainty volumes of eval_utils.full_slice_segment (eval_utils.py:176-198) and takes the queried slices in
 * datasets/data_holders.py:360; its slice selection was never published.
 * Posteriors as the library writes them: d_post [c, R] fp32, class-major, R = n_slices * V rows; 2 <= c <= 8.
 * h(p) = -sum_j p_j log p_j, evaluated in fp64 by ONE device function, a term with p_j <= 0 exactly 0.
 *
 * alq_unc_accumulate folds one dropout pass into the running sums: d_sum_p [c, R] fp64 (+)= p, d_sum_h [R] fp64 (+)= h(p)
 * (d_sum_h NULL: not kept, MC-entropy needs none).  first != 0 assigns, so the sums need no memset.  The fp64 sum of T fp32
 * values is exact.
 *
 * alq_slice_scores writes, per slice, the SUM of a per-voxel value over the slice's ROI voxels (d_scores fp64 [n_slices]) and
 * their number (d_counts int64 [n_slices]); the caller divides.  d_roi: uint8 [n_slices * V], a voxel counts when its byte is
 * non-zero; NULL: every voxel.  An empty slice: 0.0 and 0.  The value:
 *   ALQ_UNC_ENTROPY     h of the fp32 posteriors d_f32 [c, R] (no sums read)
 *   ALQ_UNC_MC_ENTROPY  h(sum_p / T)
 *   ALQ_UNC_BALD        h(sum_p / T) - sum_h / T      (exactly 0 for T = 1)
 *   ALQ_UNC_MEAN        d_f32 [R] itself (the AU_vals log-variance map)
 * Two stages: a workgroup sweeps rows_per_sweep consecutive rows at a time (whatever V is: a sweep may hold parts of two slices,
 * or many whole ones) and stores one partial per (slice, sweep) at a place of its own, then a thread per slice adds the slice's
 * partials in ascending order.  No float or double atomics; the order of every addition depends on (n_slices, V) alone, so
 * results are bit-identical from run to run.  The partials live in the context (grown by the call that needs more).
 * alq_slice_scores_geometry: out[4] = workgroup size, rows per workgroup sweep, the grid cap, partials per slice - the launch
 * arithmetic, for tests that assert the regime they name (no device call).
 * Stream-ordered, no synchronisation.  Before any launch - outputs untouched - ALQ_EINVAL: a null required pointer (ctx, the
 * outputs, the inputs of the kind), T < 1, n_slices < 1, V < 1 (R < 1), an unknown kind, a pointer not aligned to its element;
 * ALQ_EUNSUPPORTED: c outside 2 .. 8, n_slices * V (R) >= 2^31.                                                                   */
enum { ALQ_UNC_ENTROPY = 0, ALQ_UNC_MC_ENTROPY = 1, ALQ_UNC_BALD = 2, ALQ_UNC_MEAN = 3 };
int alq_unc_accumulate(alq_ctx *ctx, const float *d_post, int c, int64_t R, int first, double *d_sum_p, double *d_sum_h);
int alq_slice_scores(alq_ctx *ctx, int kind, int T, int c, int64_t n_slices, int64_t V, const double *d_sum_p, const double *d_sum_h,
                     const float *d_f32, const uint8_t *d_roi, double *d_scores, int64_t *d_counts);
int alq_slice_scores_geometry(int c, int64_t n_slices, int64_t V, int64_t *out);

/* Multi-GPU top-B merge step (no reference counterpart: the reference is one process).
 * Host function: merges the candidate (key, GLOBAL index) pairs gathered from all ranks
 * (torch.distributed all_gather over RCCL in pool_shard.merge_topB; entries with index < 0 are padding)
 * into the global top-B, ascending key (compared by bit pattern, so a NaN key sorts behind every number),
 * ties -> lower global index, so the result is identical on every rank.  For NON-NEGATIVE keys (sign bit clear: +0.0, numbers,
 * +inf, such NaNs - what |p - .5| and the other query keys are) this is the rule of alq_topk_uncertain.  It is not for the
 * rest: the merge takes -0.0 for +0.0 (the index decides between them, where the device sorts -0.0 first) and a negative key
 * sorts by its raw bits BEHIND every non-negative one, in reverse numeric order (tests/test_select_ref_host.py pins both).
 * out_idx: int64 [B]; returns the count in *n_out.                                               */
int alq_topk_merge(const double *h_keys, const int64_t *h_idx, int64_t n, int64_t B, int64_t *h_out_idx,
                   int64_t *n_out);

/* The other multi-GPU exchange (no reference counterpart): all-reduce(sum) of the L x L fp64
 * Fisher sum  sum_i A_i  over the ranks that share one pool, on RCCL over xGMI, enqueued on the context's
 * stream.  One communicator per context: rank 0 calls alq_comm_unique_id (128 bytes, host), the host side
 * distributes the id (pool_shard.attach_comm broadcasts it through torch.distributed) and every rank calls
 * alq_comm_init (collective: returns when all `world` ranks have joined).  alq_allreduce_sum reduces d_buf
 * [count] doubles IN PLACE; stream-ordered, does not synchronise.  librccl.so.1 is resolved at run time
 * (dlopen): a process without RCCL gets ALQ_EUNSUPPORTED from these three calls and nothing else changes. */
#define ALQ_COMM_ID_BYTES 128
int alq_comm_unique_id(void *h_id);
int alq_comm_init(alq_ctx *ctx, const void *h_id, int rank, int world);
int alq_comm_destroy(alq_ctx *ctx);
int alq_allreduce_sum(alq_ctx *ctx, double *d_buf, int64_t count);

/* ---- Fisher scoring --------------------------------------------------------------------- */
/* Replaces: the per-sample loop of PW_NNAL.gen_A_matrices (PW_NNAL.py:757-814): up to two
 * sess.run(model.grad_posts[j]) at batch 1, NNAL_tools.shrink_gradient(...,'sum')
 * (NNAL_tools.py:784-796) and the outer products.  d_x: [N, D,H,W,C] normalised patches.
 * d_p1_in: float [N] posteriors to branch on (what batch_eval returned, PW_NNAL.py:767) or
 * NULL to use the posteriors of this forward pass.  Outputs (any may be NULL):
 *   d_p1_out float [N]; d_g0, d_g1 double [N, L] (shrunk class-0 / class-1 gradients, zero
 *   where the reference's saturation branch skips them); d_A double [N, L, L];
 *   d_trace double [N]; d_Asum double [L, L] = sum_i A_i (overwritten, deterministic order). */
int alq_fisher(alq_model *m, const float *d_x, int N, const float *d_p1_in, double diag_load,
               float *d_p1_out, double *d_g0, double *d_g1, double *d_A, double *d_trace,
               double *d_Asum);

/* Same, on rows of a resident pool (see alq_forward_rows): the B filtered candidates `sel_inds` of
 * PW_NNAL.py:108-129 / :549-559 are passed as positions, not as a gathered copy.  d_p1_in, outputs: per row. */
int alq_fisher_rows(alq_model *m, const float *d_pool, const int64_t *d_rows, int N, const float *d_p1_in,
                    double diag_load, float *d_p1_out, double *d_g0, double *d_g1, double *d_A,
                    double *d_trace, double *d_Asum);

/* ---- parameter gradients, dropout passes, optimiser steps ------------------------------- */
/* Total number of parameters P = sum_t (w_elems + b_elems); the flat parameter / gradient vector of this API is
 * [W_0, b_0, W_1, b_1, ...] in variable-creation order and TF layouts (see alq_model_set_weights).            */
int64_t alq_model_num_params(const alq_model *m);

/* Replaces: sess.run(model.posteriors, {keep_prob: p < 1}) of the MC strategies (PW_NNAL.py:232-282: MC-entropy,
 * BALD).  Dropout (x * keep / keep_prob, NN.py:169-171) on the OUTPUT of the listed layers with a counter-based mask
 * keyed (seed, layer, first_sample + n, element): reproducible and independent of the batch split; TF's own random
 * stream is not reproducible outside TF, so the mask is this library's (the oracle restates the generator).     */
int alq_forward_dropout(alq_model *m, const float *d_x, int N, float keep_prob, uint64_t seed, int64_t first_sample,
                        const int32_t *h_drop_layers, int n_drop_layers, float *d_post, int64_t *d_pred);

/* Replaces: sess.run(model.grad_posts[str(cls)], ...) = tf.gradients(tf.log(posteriors[cls, 0]), variables)
 * (NN.py:639-645; mode 0: one full gradient per sample, the reference feeds batches of one, PW_NNAL.py:773-807) and
 * the gradient half of sess.run(model.train_step, {x, y_, keep_prob}) (NN.py:583-615; mode 1: gradient of
 * loss_scale * sum_n CE(softmax(z_n), label_n), loss_scale = 1 / batch for the reference's reduce_mean; d_labels
 * int32 [N], a label outside [0, c) contributes nothing).  per_sample = 1: d_grads [N, P]; 0: [P] summed over the
 * batch (fixed order, fp64).  d_post [c, N] and d_loss (mean CE of the batch, mode 1) optional.  Dropout as above
 * (keep_prob = 1: none).  Never on the 'sum'-shrink scoring path, which forms no weight gradient (alq_fisher).  */
int alq_param_grads(alq_model *m, const float *d_x, int N, int mode, int cls, const int32_t *d_labels,
                    float loss_scale, float keep_prob, uint64_t seed, int64_t first_sample,
                    const int32_t *h_drop_layers, int n_drop_layers, int per_sample, float *d_grads,
                    float *d_post, double *d_loss);

/* Replaces: the per-sample, per-class session.run(model.grad_log_posts) and the squared sums of the expected-gradient-length
 * query (NNAL.py:234-285).  Per-sample squared norms of parameter gradients, never materialising them.  cls = -1:
 * u = d(z0 - z1)/dtheta (two-class nets only, ALQ_EINVAL otherwise; d log p0 = p1 u, d log p1 = -p0 u); cls in [0, c):
 * d log posteriors[cls, n] / dtheta; d_cls [N] int32 (optional, entries in [0, c)) overrides cls per sample.
 * d_sq [N, 2L] double: [n][2t] = ||dW_t||^2, [n][2t+1] = ||db_t||^2, all L parameterised layers in creation order.
 * d_post [c, N] optional.  keep_prob 1.  Weight norms of conv / conv_transpose layers on the fp32 matrix cores (exact fp32
 * products, fp32 accumulation in two levels, fp64 squares); fc layers by the rank-one identity ||delta||^2 ||a||^2.
 * Every row depends on its own sample only: bit-identical whatever the batch and from run to run.                    */
int alq_grad_sqnorms(alq_model *m, const float *d_x, int N, int cls, const int32_t *d_cls,
                     float *d_post, double *d_sq);

/* Replaces: the Hessian-vector product behind the reference's influence functions - Influence.get_hess_vec_product /
 * hessian_vector_product (Influence.py:64-166: tf.gradients of <grad L, stop_gradient(v)>, the Pearlmutter double-backward),
 * what sess.run(model.hess_vecp) and PW_NN.batch_eval(..., 'hess_vecp') (PW_NN.py:467, :532-533) return and
 * PW_sample_influence (Influence.py:369-453) feeds to scipy's Newton-CG.  d_hv [P] double = H v, H = the Hessian of
 * loss_scale * sum_n CE(softmax(z_n), label_n) with respect to the flat parameter vector [W_0, b_0, W_1, b_1, ...] (order and
 * layouts of alq_param_grads; d_v [P] float on the device in the same order; d_labels int32 [N], a label outside [0, c)
 * contributes nothing; keep_prob 1).  The EXACT R-operator, not a Gauss-Newton product.  The ordinary forward pass with
 * everything kept fixes the ReLU signs and the max-pool arg-max; on those decisions the call re-evaluates, in fp64 tensors of
 * its own (csrc/hvp.hip): the activations, the posteriors and the first-order cotangents; the tangent forward pass (Rz_l =
 * op(a_{l-1}; V_l) + c_l + op(Ra_{l-1}; W_l), ReLU by the stored sign, max-pool at the stored arg-max, 'con' skips
 * concatenated); Rdelta = loss_scale (diag(p) - p p^T) Rz at the logits; one backward sweep of the tangent cotangent; and the
 * two-term weight products.  Sums in a fixed order, no [N, P] buffer, no atomics - bit-identical from run to run, and exactly
 * linear in v and in loss_scale under powers of two.
 * h_layer_on (host, [L] bytes, or NULL = every layer; the reference's Hess_layers): a layer that is switched off is held
 * constant - its entries of d_v are never read, its entries of d_hv are written as zeros (left alone when accumulate is set).
 * accumulate = 1: d_hv += H v, so a set larger than max_batch is a sequence of calls with loss_scale = 1 / n_total.
 * d_loss (optional): the scaled loss of the call.  The workspaces - four fp64 tensors per layer output (activation, cotangent
 * and their two tangents, sized for max_batch), the slab partials of the conv weight products (at most 32 MiB), the fp64
 * posteriors and an fp32 copy of the weights in the TF layout - are allocated on the device by the first call.  Until a call
 * has uploaded them, a model keeps on the host the weight arrays alq_model_set_weights was given for conv / conv_transpose and
 * wide fc layers (their engines hold split forms only); skinny fc layers and layers set by alq_model_set_weights_device are
 * read from their resident fp32 copies.  Stream-ordered; synchronises only to upload weights set since the last call.
 * ALQ_EINVAL: null d_x / d_labels / d_v / d_hv, N outside [1, max_batch], weights not set.                               */
int alq_hess_vecp(alq_model *m, const float *d_x, int N, const int32_t *d_labels, float loss_scale, const float *d_v,
                  const uint8_t *h_layer_on, int accumulate, double *d_hv, double *d_loss);

/* Replaces: tf.train.GradientDescentOptimizer / AdamOptimizer .minimize (NN.py:591-615) on flat device vectors:
 * theta -= lr g;  Adam (TF-1.x defaults are the caller's: beta1 .9, beta2 .999, eps 1e-8), step count t >= 1:
 * lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), m = b1 m + (1-b1) g, v = b2 v + (1-b2) g^2,
 * theta -= lr_t m / (sqrt(v) + eps).  The updated vector goes back through alq_model_set_weights.              */
int alq_sgd_step(alq_ctx *ctx, float *d_theta, const float *d_grad, int64_t n, float lr);
int alq_adam_step(alq_ctx *ctx, float *d_theta, const float *d_grad, float *d_m, float *d_v, int64_t n, float lr,
                  float beta1, float beta2, float eps, int64_t t);
/* ---- the training objectives of NN_extended.CNN and the RMSProp step (csrc/loss.hip) ---------------------------------------- */
/* What differs between the objectives of NN_extended.get_loss is the cotangent at the logits and the reported value; this
 * struct describes one.  Per sample n with label y, posterior column p (fp32, as the head wrote it) and pt = p[y]:
 *   ALQ_LOSS_CE       w = [0 <= y < c] * class_w[y] * sample_w[n] * f,  f = (1 - pt)^gamma with focal_gamma > 0 (1 - pt formed in
 *                     fp32), else 1;  l = -w log pt;  row_j = s [labelled] class_w[y] sample_w[n] (p_j - delta_jy)
 *                     ((1 - pt)^gamma - gamma (1 - pt)^(gamma - 1) pt log pt): the focal weight is differentiated, as TF does
 *                     (no stop_gradient); at pt == 1.0f the focal row is exactly zero and w = 0.  With unit weights and no focal
 *                     term the row has the bits alq_param_grads mode 1 writes.
 *   ALQ_LOSS_CE_SOFT  targets t [c, N]: l = -sum_j t_j log p_j;  row_j = s (p_j sum_k t_k - t_j).
 *   ALQ_LOSS_GCE      pc = clip(p, 1e-4, 1 - 1e-4): l = (1 / c) sum_j t_j (1 - pc_j^q) / q;
 *                     row_k = -(s / c) sum_j t_j [1e-4 <= p_j <= 1 - 1e-4] p_j^q (delta_jk - p_k).
 *   d_old_logits != NULL adds the learning-without-forgetting term (model_utils.get_LwF): tau = softmax(o / T),
 *                     pi = softmax(z / T) formed FROM THE FP32 POSTERIORS (pi_j ~ p_j^(1/T), normalised; log p as below), not
 *                     from the logits: l' = -sum_j tau_j log pi_j, row_j += s' (pi_j - tau_j) / T, unlabelled samples included.
 *                     (Exact while no posterior underflows fp32, i.e. while the logits of a sample spread by less than 87.)
 * -log p is log((double)max(p, 1e-38f)) throughout.  s = loss_scale and s' = lwf_scale are the caller's (1 / divisor).
 * focal_gamma <= 0 (or negative: off) leaves the focal term out.  All pointers are device pointers; NULL = absent.
 * Statistics d_stats3 (double [3], device): sum_n l_n unscaled; the number of samples whose weight w is not zero (TF's
 * SUM_BY_NONZERO_WEIGHTS divisor; N for the two soft kinds); sum_n l'_n.  Per-workgroup partials in a fixed tree, summed in
 * workgroup order by a second launch: no atomics, bit-identical from run to run.                                          */
enum { ALQ_LOSS_CE = 0, ALQ_LOSS_CE_SOFT = 1, ALQ_LOSS_GCE = 2 };
typedef struct alq_loss_t {
    int32_t kind;
    float focal_gamma;            /* < 0: off */
    float gce_q;
    float lwf_T;
    const float *d_class_w;       /* [c] */
    const float *d_sample_w;      /* [N] */
    const float *d_targets;       /* [c, N] */
    const float *d_old_logits;    /* [c, N] */
} alq_loss_t;

/* Replaces: sess.run(model.loss, ...) of an NN_extended.CNN whose loss is one of the above (NN_extended.py:1221-1277;
 * model_utils.py:98-135), given the posteriors [c, N] of a forward pass: the three statistics alone, nothing else written.
 * d_labels int32 [N] (required for ALQ_LOSS_CE; a label outside [0, c) is an unlabelled sample).  ALQ_EINVAL: null ctx /
 * d_post / loss / d_stats3, c < 1, N < 1, an unknown kind, CE without labels, CE_SOFT or GCE without targets, GCE with
 * gce_q == 0, old logits with lwf_T <= 0.                                                                             */
int alq_loss_stats(alq_ctx *ctx, const float *d_post, int c, int N, const int32_t *d_labels, const alq_loss_t *loss,
                   double *d_stats3);

/* Replaces: the gradient half of sess.run(model.train_step / model.LwF_train_step, ...) of an NN_extended.CNN
 * (optimizer.compute_gradients(model.loss), NN_extended.py:1380-1449; model_utils.py:98-135): alq_param_grads mode 1 with the
 * cotangent of `loss` at the logits - same forward pass, dropout arguments, backward sweep, weight products and [P] layout
 * (summed over the batch).  d_post [c, N] and d_stats3 optional.  ALQ_EINVAL: as alq_loss_stats, null m / d_x / d_grads,
 * N outside [1, max_batch].                                                                                              */
int alq_param_grads_loss(alq_model *m, const float *d_x, int N, const int32_t *d_labels, const alq_loss_t *loss,
                         float loss_scale, float lwf_scale, float keep_prob, uint64_t seed, int64_t first_sample,
                         const int32_t *h_drop_layers, int n_drop_layers, float *d_grads, float *d_post, double *d_stats3);

/* Replaces: tf.train.RMSPropOptimizer(lr, decay, momentum, epsilon).apply_gradients (NN_extended.py:1399-1404; not centred)
 * on flat device vectors: ms = decay ms + (1 - decay) g^2; mom = momentum mom + lr g / sqrt(ms + eps); theta -= mom.
 * TF 1.x starts the rms slot at ones and the momentum slot at zeros: the caller allocates d_ms / d_mom that way.           */
int alq_rmsprop_step(alq_ctx *ctx, float *d_theta, const float *d_grad, float *d_ms, float *d_mom, int64_t n, float lr,
                     float decay, float momentum, float eps);

/* ---- mean-teacher consistency training of a fully-convolutional model (NN_extended.py:913-926, :1337-1396, :1535-1560) ----
 * The student's posteriors p and the teacher's q, both class-major planes [c, R] over R = N V voxels, 2 <= c <= 8.  Per voxel
 *   div = mean_j (p_j - q_j)^2 (ALQ_MT_L2)   or   -sum_j p_j log q_j (ALQ_MT_CE; log as in alq_loss_t)
 * and the row of  loss_scale * sum_v l_v + k' * sum_v div_v  at the logits, l the ALQ_LOSS_CE objective of `loss` (class, voxel
 * and focal weights; targets and old logits must be NULL):
 *   row_k = [the row alq_param_grads_loss writes at loss_scale] + cons_scale p_k (d_k - sum_j p_j d_j),  d = p - q,
 * cons_scale = 2 k' / c, for ALQ_MT_L2 on every voxel, labelled or not; ALQ_MT_CE adds nothing to a row (TF 1.x's
 * softmax_cross_entropy_with_logits does not differentiate its labels and the teacher sits behind stop_gradient).  The
 * consistency term is formed in fp64 from the fp32 posteriors and is added before the one rounding to fp32; with
 * cons_scale == 0 the rows have the bits alq_param_grads_loss writes.  Statistics d_stats3 (double [3], device): sum_v l_v
 * unscaled, the number of voxels whose weight is not zero, sum_v div_v.  No atomics: bit-identical from run to run.        */
enum { ALQ_MT_L2 = 0, ALQ_MT_CE = 1 };
/* Voxels one sweep of the capped grid of the cotangent kernel covers on its 16-byte path (more: the lanes grid-stride). */
int64_t alq_mt_trip_voxels(void);
/* Replaces: tf.gradients of model.loss = L + cons_coeff * cons at the logits (get_FCN_loss with MT_SSL, NN_extended.py:1353-1396;
 * measure_output_perturbation, :1535-1560), given both posteriors: d_rows [R, c] and the statistics.  For tests and tools (a
 * training step goes through alq_param_grads_loss_mt).  ALQ_EINVAL before any launch: a null pointer (d_teacher_post included),
 * c outside [2, 8], R < 1, an unknown measure, a loss that is not ALQ_LOSS_CE without targets / old logits.                      */
int alq_mt_cotangent(alq_ctx *ctx, const float *d_post, const float *d_teacher_post, int c, int64_t R, const int32_t *d_labels,
                     const alq_loss_t *loss, float loss_scale, float cons_scale, int measure, float *d_rows, double *d_stats3);
/* Replaces: sess.run(model.loss / model.labeled_loss / model.cons_loss, ...) of such a model: the same pass, statistics only. */
int alq_mt_stats(alq_ctx *ctx, const float *d_post, const float *d_teacher_post, int c, int64_t R, const int32_t *d_labels,
                 const alq_loss_t *loss, int measure, double *d_stats3);
/* Replaces: the gradient half of sess.run(model.train_step, ...) with MT_SSL (NN_extended.py:1006-1008, :1353-1396):
 * alq_param_grads_loss for a fully-convolutional model with the cotangent above - same forward pass, dropout arguments, head
 * backward, backward sweep, weight products and [P] layout.  d_teacher_post [c, N V]: the teacher's posteriors of its own
 * (perturbed) input, constants of the step.  ALQ_EINVAL: as alq_mt_cotangent and alq_param_grads_loss; ALQ_EUNSUPPORTED: an
 * fc-head model (the reference's axes need an output map).  Nothing is launched before the checks pass.                      */
int alq_param_grads_loss_mt(alq_model *m, const float *d_x, int N, const int32_t *d_labels, const alq_loss_t *loss,
                            float loss_scale, const float *d_teacher_post, int measure, float cons_scale, float keep_prob,
                            uint64_t seed, int64_t first_sample, const int32_t *h_drop_layers, int n_drop_layers, float *d_grads,
                            float *d_post, double *d_stats3);
/* ---- aleatoric uncertainty for unlabelled voxels (AU_4U, NN_extended.py:265-288, :1376-1383, :1551-1554) ----
 * The head of a fully-convolutional model has c + 1 channels: c classes and, behind a ReLU, a per-voxel log-variance a >= 0.
 * With e = exp(-a) the consistency value of a voxel is  cons = div e + kappa a / 2  (kappa = AU_log_rel_coeff; div as above,
 * over the c posteriors; the teacher's own log-variance is not read), and the rows [R, c + 1] at the student's logits are
 *   k < c:  [the labelled row, on the c clean logits] + cons_scale e p_k (d_k - sum_j p_j d_j)   (ALQ_MT_L2; ALQ_MT_CE: no term)
 *   c:      a > 0 ? au_scale (kappa / 2 - div e) : 0                                               (TF's ReluGrad; both measures)
 * formed in fp64 from the fp32 planes and rounded once.  With d_au all zero and kappa = 0 the columns below c and the statistics
 * have the bits of alq_mt_cotangent at the same cons_scale and column c is 0.  Statistics: sum_v l_v, the non-zero weights,
 * sum_v cons_v.  No atomics: bit-identical from run to run.
 * alq_model_set_aleatoric(m, on): the model's head is read that way from here on: alq_forward and alq_forward_dropout write
 * d_post [c, N V] and d_pred over the c classes, alq_param_grads_loss and alq_param_grads_loss_mt return ALQ_EUNSUPPORTED before
 * any launch.  ALQ_EUNSUPPORTED unless the model has a 1x1 conv head of 3 .. 8 channels.                                        */
int alq_model_set_aleatoric(alq_model *m, int on);
/* Replaces: sess.run(model.posteriors / model.AU_vals / model.output, ...) of such a model (eval_utils.py:147-198): one forward
 * pass - dropout arguments as alq_forward_dropout, keep_prob = 1: none - into d_post [c, N V] (or NULL), d_pred (or NULL),
 * d_au [N V] and d_logits [N V, c + 1] (or NULL).  ALQ_EINVAL: a null m / d_x / d_au, N outside [0, max_batch];
 * ALQ_EUNSUPPORTED: a model without alq_model_set_aleatoric.                                                                    */
int alq_forward_au(alq_model *m, const float *d_x, int N, float keep_prob, uint64_t seed, int64_t first_sample,
                   const int32_t *h_drop_layers, int n_drop_layers, float *d_post, int64_t *d_pred, float *d_au, float *d_logits);
/* Voxels one sweep of the capped grid of the aleatoric cotangent kernel covers on its 16-byte path. */
int64_t alq_mt_au_trip_voxels(void);
/* alq_mt_cotangent / alq_mt_stats with the log-variance plane d_au [R]: d_rows [R, c + 1].  ALQ_EINVAL before any launch: a null
 * d_au, c outside [2, 7], and the conditions of alq_mt_cotangent.  R % 4 != 0 or a base that is not 16-byte aligned (d_au
 * included): the guarded one-voxel path.                                                                                        */
int alq_mt_cotangent_au(alq_ctx *ctx, const float *d_post, const float *d_teacher_post, const float *d_au, int c, int64_t R,
                        const int32_t *d_labels, const alq_loss_t *loss, float loss_scale, float cons_scale, float au_scale,
                        float au_log_rel_coeff, int measure, float *d_rows, double *d_stats3);
int alq_mt_stats_au(alq_ctx *ctx, const float *d_post, const float *d_teacher_post, const float *d_au, int c, int64_t R,
                    const int32_t *d_labels, const alq_loss_t *loss, float au_log_rel_coeff, int measure, double *d_stats3);
/* alq_param_grads_loss_mt for a model with alq_model_set_aleatoric: the head's forward launch writes the log-variances, the rows
 * above go through the existing head backward with c + 1 columns.  d_teacher_post [c, N V]; d_post [c, N V] optional.  The caller
 * passes cons_scale = coeff 2 / (c V) and au_scale = coeff / V.  ALQ_EINVAL: as alq_mt_cotangent_au and alq_param_grads_loss;
 * ALQ_EUNSUPPORTED: a model without the flag.  Nothing is launched before the checks pass.                                      */
int alq_param_grads_loss_mt_au(alq_model *m, const float *d_x, int N, const int32_t *d_labels, const alq_loss_t *loss,
                               float loss_scale, const float *d_teacher_post, int measure, float cons_scale, float au_scale,
                               float au_log_rel_coeff, float keep_prob, uint64_t seed, int64_t first_sample,
                               const int32_t *h_drop_layers, int n_drop_layers, float *d_grads, float *d_post, double *d_stats3);
/* Replaces: sess.run(model.ema_apply) (tf.train.ExponentialMovingAverage.apply, NN_extended.py:913-926): per element
 * shadow -= (shadow - theta) * (1 - decay), every operation rounded to fp32 (1 - decay included).  ALQ_EINVAL: null pointer
 * with n > 0, n < 0, decay outside [0, 1].                                                                                  */
int alq_ema_step(alq_ctx *ctx, float *d_shadow, const float *d_theta, int64_t n, float decay);
/* Replaces: perturb_input (NN_extended.py:1337-1351) on a channels-last batch [N, H, W, C]: Gaussian noise of standard
 * deviation noise_std, then - rotate != 0 - tf.contrib.image.rotate(x, angle): nearest neighbour about the image centre,
 * counter-clockwise, zero outside.  One gather: out[n, y, x, ch] = in[n, ys, xs, ch] + noise_std * z(n, ys, xs, ch) with, in fp32,
 *   xo = ((W-1) - (cos a (W-1) - sin a (H-1))) / 2,  yo = ((H-1) - (sin a (W-1) + cos a (H-1))) / 2,
 *   ys = round(sin a x + cos a y + yo),  xs = round(cos a x - sin a y + xo)   (half away from zero; outside the image: 0).
 * z: Box-Muller on two 24-bit uniforms of the dropout masks' counter-based generator keyed (seed, a tag no layer has, sample id
 * first_sample + n, source element in memory order): independent of the batch split.  A 3-D batch [N, D, H, W, C] takes the
 * call with H = D * H and rotate = 0.  d_out may be d_x when rotate == 0.  ALQ_EINVAL: null pointer, a size below 1,
 * noise_std < 0, a rotation in place.                                                                                        */
int alq_perturb_input(alq_ctx *ctx, const float *d_x, float *d_out, int N, int H, int W, int C, float noise_std, uint64_t seed,
                      int64_t first_sample, int rotate, float angle);

/* Replaces: the accumulation loop of model_utils.diagonal_Fisher (model_utils.py:294-330):
 * d_acc[i] += sum_n d_grads[n, i]^2 (fp64).                                                                    */
int alq_sq_accum(alq_ctx *ctx, const float *d_grads, int64_t per_sample_len, int N, double *d_acc);

/* ---- image-level multi-class Fisher query (NNAL.py:312-464) --------------------------------------------------- */
/* Replaces: NNAL_tools.shrink_gradient(grads[str(j)], 'sum') (NNAL_tools.py:784-796) on the per-sample gradient lists that
 * session.run(nz_classes_grads) returns (NNAL.py:381-397), with the gradients staying on the device: d_grads [N, P] rows as
 * alq_param_grads(mode 0, per_sample 1) writes them, h_layer_elems [L] = |W_t| + |b_t| (host; their sum must be P);
 * d_out [N, L] double: (sum of layer t's entries) / (|W_t| + |b_t|), fp64 sums in a fixed order.                        */
int alq_shrink_sum(alq_ctx *ctx, const float *d_grads, int N, int64_t P, const int64_t *h_layer_elems, int L, double *d_out);
/* Replaces: the same per-sample, per-class gradient lists and their shrink (NNAL.py:381-405), without forming a gradient:
 * d_g [N, J, L] double, d_g[n][j][t] = (sum of layer t's entries of d log posteriors[d_cls[j][n], n] / d theta) /
 * (|W_t| + |b_t|), the quotient in fp64 as in alq_shrink_sum.  d_cls [J][N] int32 on the device: the class of slot j for
 * every sample, 1 <= J <= 64; any class count from 2 to 64; N <= max_batch; keep_prob 1.  One forward pass, one softmax,
 * one field launch per parameterised layer (the class-independent factor of the sum: box / transposed box of the input's
 * channel sums + 1, fc: sum of the input + 1), then per slot the logit cotangent e_j - p, the general backward-data sweep
 * with the fused mask + channel-sum + dot kernel of csrc/lsum.hip per layer, and a fixed-order finish: no weight gradient,
 * no [N, P] buffer, no weight-gradient workspace.  d_post [c, N] optional.  A class outside [0, c) gives ALQ_EINVAL and
 * nothing is written (the slots are checked on the device first: one 4-byte flag read, which synchronises the stream).
 * Every row depends on its own sample only: bit-identical whatever the batch, the slot position and from run to run.   */
int alq_class_layer_sums(alq_model *m, const float *d_x, int N, int J, const int32_t *d_cls, float *d_post, double *d_g);

/* Replaces: model_utils.diagonal_Fisher (model_utils.py:294-330) without per-sample gradient rows:
 * d_acc[i] += sum_n (d log posteriors[d_cls[n], n] / d theta_i)^2, theta the flat vector [W_0, b_0, W_1, b_1, ...] in the order
 * and TF layouts of alq_param_grads.  d_cls [N] int32 on the device, entries in [0, c): checked on the device before anything
 * is written (one 4-byte flag read, which synchronises the stream); a class outside the range gives ALQ_EINVAL and d_acc is
 * left alone.  d_acc [P] double: the call always ADDS, the caller zeroes it; a set larger than max_batch is a sequence of calls.
 * keep_prob 1.  Conv / conv_transpose weights: every 16 x 16 tile of a sample's weight gradient is held in registers on the
 * fp32 matrix cores for the sample's voxel sweep (exact fp32 products, fp32 accumulation in two levels), squared in fp64 and
 * added to fp64 accumulators that leave the workgroup after its last sample; biases from fp64 channel sums; fc layers as
 * sum_n delta[n, o]^2 a[n, f]^2 in fp64.  No [N, P] buffer and no atomics: every sum has a fixed order, the result is
 * bit-identical from run to run.  Scratch (allocated by the first call): the largest of one conv layer's sample-group
 * partials and max_batch x (widest layer) doubles.  ALQ_EINVAL: null argument, N outside [1, max_batch].                   */
int alq_diag_fisher(alq_model *m, const float *d_x, int N, const int32_t *d_cls, double *d_acc);

/* Replaces: model_utils.keep_k_largest_from_LoV / threshold_LoV (model_utils.py:54-96) on a flat device vector.
 * alq_topk_mask: d_mask [n] float = 1 on exactly k entries, the k largest of d_v [n] double, 0 elsewhere; entries equal to the
 * k-th largest value are taken in ascending index order (the reference's argsort leaves tie order open).  Numeric order for
 * any finite double, -0.0 equal to +0.0.  k = 0: all zeros; k = n: all ones; k < 0 or k > n: ALQ_EINVAL.  A radix select
 * on the bit patterns (8 histogram passes over d_v) and one ordered pass; nothing is sorted.  d_work: device scratch of
 * alq_topk_mask_work_bytes(n) bytes (about 1 MiB + n / 512 bytes).  Stream-ordered, no synchronisation.
 * alq_threshold_mask: d_mask[i] = d_v[i] >= thr ? 1 : 0.                                                                      */
size_t alq_topk_mask_work_bytes(int64_t n);
int alq_topk_mask(alq_ctx *ctx, const double *d_v, int64_t n, int64_t k, float *d_mask, void *d_work);
int alq_threshold_mask(alq_ctx *ctx, const double *d_v, int64_t n, double thr, float *d_mask);
/* Replaces: the accumulation `Ai += np.outer(g_j, g_j) / new_posts[j] + np.eye(A_size) * 1e-5` over the selected classes
 * (NNAL.py:399-409).  d_g [N, c, L] shrunk class gradients, d_w [N, c] = 1 / new_posts for the classes the reference
 * keeps (posterior >= 1e-6; the ten largest when ten or more remain, :381-394) and 0 for the others - host logic on the
 * posteriors, like the reference's -, d_diag [N] = (number of kept classes) * 1e-5; d_A [N, L, L] double.             */
int alq_fisher_classes(alq_ctx *ctx, const double *d_g, const double *d_w, const double *d_diag, int N, int c, int L,
                       double *d_A);

/* ---- feature similarities (representativeness strategies) -------------------------------------------- */
/* Replaces: the NumPy similarity blocks of query_multimg 'rep-entropy' (PW_NNAL.py:318-327: norms, dots = F.T @ F_u,
 * sims = dots / outer(norms)) and 'core-set' (:386-425, :437-441).  Features are fp32 rows [samples, f] as
 * alq_forward returns them; accumulation is fp64 like the reference's float64 arrays.
 *   alq_row_norms      d_norms[i] = ||A[i, :]||
 *   alq_cosine_sims    d_C[i, j] = <A[i], B[j]> / (na[i] nb[j])   (both norm vectors null: plain dot products)
 *   alq_colsum_max     d_out[j] = sum_i max(d_cmax[i], S[i, j]) over the rows with d_skip[i] == 0 (either may be null):
 *                      the representativeness score of every candidate column in ONE pass (PW_NNAL.py:333-338 scores one
 *                      candidate per Python iteration); fixed summation order; d_work: alq_colsum_work_bytes(n, b) bytes
 *   alq_take_colmax    d_v[i] = max(d_v[i], S[i, j])  (first != 0: d_v[i] = S[i, j]): the running row maxima after a pick
 *   alq_fold_rowmax    d_v[j] = max(d_v[j], max_i S[i, j]) for a [t, n] block (core-set's labelled-set maxima, :420-425)
 * Non-finite values: a zero-norm row of A (of B) makes its row (its column) of d_C NaN, 0 / 0 as in the reference's NumPy.  The
 * three max kernels take every maximum with fmax, which IGNORES a NaN operand (fmax(NaN, x) = x; NaN only when both are), where
 * the reference's np.max / np.maximum propagate it: alq_colsum_max sums fmax(d_cmax[i], S[i, j]) (without d_cmax a NaN entry
 * makes its column's sum NaN), alq_take_colmax with first != 0 copies the column, NaN included, and otherwise keeps d_v[i] over
 * a NaN entry, alq_fold_rowmax skips NaN entries and replaces a NaN d_v[j] by the column's maximum.  DESIGN.md, "Zero feature
 * vectors", says what that means for the two queries. */
int alq_row_norms(alq_ctx *ctx, const float *d_A, int64_t n, int f, double *d_norms);
int alq_cosine_sims(alq_ctx *ctx, const float *d_A, int64_t n, const float *d_B, int b, int f, const double *d_na,
                    const double *d_nb, double *d_C);
size_t alq_colsum_work_bytes(int64_t n, int b);
int alq_colsum_max(alq_ctx *ctx, const double *d_S, int64_t n, int b, const double *d_cmax,
                   const unsigned char *d_skip, double *d_out, void *d_work);
int alq_take_colmax(alq_ctx *ctx, const double *d_S, int64_t n, int b, int j, int first, double *d_v);
int alq_fold_rowmax(alq_ctx *ctx, const double *d_S, int t, int64_t n, double *d_v);

/* ---- region primitives: local variance maps and per-segment minima (csrc/region.hip) ------------------------------- */
/* Replaces: patch_utils.get_vars_2d (patch_utils.py:794-826) applied to every slice of a subject, as PW_NNAL.get_HV_inds does
 * for the `ps-random` queries (PW_NNAL.py:632-669), on a volume that is already resident for alq_gather_normalize.
 * d_vol: one zero-padded C-order volume, float or double (vol_is_f64 = 1); pad_dims its padded shape, rads the padding radii;
 * the map is defined on the un-padded box [H, W, S] = pad_dims - 2 rads.  For every slice z and pixel (i, j):
 * t = trunc(v) as an integer, S1 = sum t and S2 = sum t^2 (64-bit integer sums) over rows [i - d/2, i + (d-1)/2] x columns
 * [j - d/2, j + (d-1)/2] (integer division) clipped to the slice, var = double(S2) / double(d d) - (double(S1) / double(d d))^2,
 * every operation rounded on its own.  Bit-identical to the reference's scipy statement whenever all values are finite, >= 0
 * and trunc(max)^2 d^2 < 2^53 (the caller checks; beyond that the reference itself is inexact).
 * d_inds NULL: d_out = the whole map, double [H, W, S] in C order (n is ignored).  Otherwise d_out[q], q < n, = the map at
 * un-padded raveled index d_inds[q] (only those windows are formed; an index outside the box gives NaN and reads nothing).
 * ALQ_EINVAL: null argument, d outside [1, 65], a radius that leaves no voxel.  Stream-ordered, no synchronisation.          */
int alq_local_var2d(alq_ctx *ctx, const void *d_vol, int vol_is_f64, const int64_t pad_dims[3], const int32_t rads[3], int d,
                    const int64_t *d_inds, int64_t n, double *d_out);
/* Replaces: the regionprops(slice, score_img) 'min_intensity' loop of PW_NNAL.superpix_scoring (PW_NNAL.py:944-1021).
 * d_labels: int32 over-segmentation [H, W, S] = dims, C order; d_inds: int64 [n] raveled indices into it, d_scores: double [n].
 * d_table: double [S, n_labels]; the call fills it with +inf, then entry (z, l) becomes the minimum of the scores of the
 * scored voxels of slice z whose label is l, for 1 <= l < n_labels.  Label 0 (background), a label outside the range and an
 * index outside the volume are skipped: nothing is stored for them.  The minimum is taken with integer atomics on an
 * order-preserving key of the double, so the table is bit-identical from run to run (-0.0 orders below +0.0).
 * NaN scores are outside the contract (their keys order by bit pattern).  Stream-ordered, no synchronisation.                */
int alq_segment_min(alq_ctx *ctx, const int32_t *d_labels, const int64_t dims[3], int32_t n_labels, const int64_t *d_inds,
                    const double *d_scores, int64_t n, double *d_table);

/* ---- connected components, largest component, hole filling (csrc/ccl.hip) -------------------------------------------- */
/* Replaces: post_processing.connected_component_analysis_3d (skimage.measure.label + the largest component) and
 * post_processing.fill_holes (scipy's binary_fill_holes), the two steps eval_utils.get_full_segs(post_process=True) applies to
 * a segmentation before scoring or saving it.  d_seg: uint8 volume [H, W, S] = dims in C order (z contiguous; S = 1: a 2-D
 * image), H W S < 2^31.  connectivity 6 / 18 / 26: face, face + edge, face + edge + corner neighbours.
 *   alq_cc_label         d_labels int32 [H, W, S]: for a selected voxel (!= 0, or == 0 with select_zero) the smallest raveled
 *                        index of its component, -1 for every other voxel.  A pure function of the input: atomic-min
 *                        union-find whose roots are minima, the same bits whatever order the workgroups run in.
 *   alq_cc_keep_largest  d_out uint8 [H, W, S] = 1 on the largest component of the non-zero voxels, 0 elsewhere.  Sizes are
 *                        exact integer sums; among equal sizes the component whose first voxel comes first in C order wins.
 *                        skip_origin: the component that holds voxel 0 is no candidate.  d_info int64 [4] = (number of
 *                        candidates, the winner's root or -1, its size, number of non-zero voxels); without a candidate
 *                        d_out is all zero.
 *   alq_fill_holes       d_out = 1 where d_seg != 0 or where the voxel belongs to a 6-connected component of the zero voxels
 *                        that touches none of the six faces of the volume (binary_fill_holes' default structure).
 *                        d_info int64 [4] = (enclosed background components, voxels filled, 0, 0).
 * d_out may be d_seg (in place).  d_work: alq_cc_work_bytes(dims) bytes (64 + 8 per voxel; 0 for dims the calls refuse), 8-byte
 * aligned like d_info.  ALQ_EINVAL before any launch: a null pointer, another connectivity, an axis below 1, 2^31 voxels or
 * more.  Stream-ordered, no synchronisation.                                                                                 */
size_t alq_cc_work_bytes(const int64_t dims[3]);
int alq_cc_label(alq_ctx *ctx, const uint8_t *d_seg, const int64_t dims[3], int connectivity, int select_zero, int32_t *d_labels);
int alq_cc_keep_largest(alq_ctx *ctx, const uint8_t *d_seg, const int64_t dims[3], int connectivity, int skip_origin, uint8_t *d_out,
                        int64_t *d_info, void *d_work);
int alq_fill_holes(alq_ctx *ctx, const uint8_t *d_seg, const int64_t dims[3], uint8_t *d_out, int64_t *d_info, void *d_work);
/* Sizes of every component and relabelling by a table (datasets/lesion_utils.py: find_lesion_components,
 * drop_lesions_with_threshold).  d_labels: int32 [n] as alq_cc_label wrote it (the root of the voxel's component, or -1).
 *   alq_cc_sizes    d_sizes int32 [n]: at every root voxel the size of its component, 0 elsewhere (the call zeroes it).  One
 *                   atomic per run of equal labels inside a wave, the runs of one root summed in the wave first: exact.
 *   alq_cc_relabel  exactly one output: d_out_i32[v] = label < 0 ? 0 : d_table[label] (d_table int32 [n], e.g. ranks), or
 *                   d_out_u8[v] = label >= 0 && d_sizes[label] >= min_size.  A label of n or above reads nothing and gives 0.
 * 0 <= n < 2^31 (n = 0: nothing is done).  ALQ_EINVAL: a null pointer, both or neither outputs, the table its output needs
 * missing, n out of range.  Stream-ordered, no synchronisation.                                                              */
int alq_cc_sizes(alq_ctx *ctx, const int32_t *d_labels, int64_t n, int32_t *d_sizes);
int alq_cc_relabel(alq_ctx *ctx, const int32_t *d_labels, int64_t n, const int32_t *d_table, const int32_t *d_sizes, int32_t min_size,
                   int32_t *d_out_i32, uint8_t *d_out_u8);

/* ---- surface distances: surface voxels, exact distance transform, masked reductions (csrc/edt.hip) -------------------- */
/* The primitives of the boundary metrics (Hausdorff, its percentile form, average symmetric surface distance, modified
 * Hausdorff; surfdist.py states each of them in NumPy and builds the metrics).  Volumes are [H, W, S] = dims in C order (z
 * contiguous; S = 1: a 2-D image).  Every call is stream-ordered, does not synchronise, and validates before any launch.
 *   alq_surface_mask   d_out uint8 [H, W, S] = 1 on a foreground voxel that has a 6-neighbour which is background or outside the
 *                      volume, 0 elsewhere.  Foreground: d_seg != 0 for label < 0, else d_seg == label (0 .. 255).  An axis of
 *                      extent 1 has no neighbours and is ignored: a one-slice volume is the 4-neighbour 2-D case, a 1x1x1
 *                      foreground voxel is no surface voxel.  d_out may NOT be d_seg.  H W S < 2^31.
 *   alq_edt_sq         d_out double [H, W, S] = the exact squared Euclidean distance transform to the non-zero voxels of d_feat
 *                      (uint8), +inf everywhere when there is none.  Defined as three line passes over g = 0 on a feature voxel,
 *                      +inf elsewhere, in the order z, w, h: g[x] = min over x' of (g[x'] + spacing2 * (double)((x - x')^2)),
 *                      the product rounded, then the sum rounded - equal to the minimum over the feature voxels of
 *                      ((s2z dz^2 + s2w dw^2) + s2h dh^2) in that association, to the bit.  spacing2 = the SQUARED voxel
 *                      spacings (h, w, z), host doubles, finite and > 0.  Every axis is 1 .. alq_edt_max_axis() = 1024 (a
 *                      staged tile of 8 whole lines of the longest axis is 64 KiB of LDS).  d_work: alq_edt_work_bytes(dims)
 *                      bytes (0 for dims the call refuses), d_out 8-byte aligned.  No atomics.
 *   alq_edt_geometry   host arithmetic: out[4] = lines per tile of the z pass, z columns per tile of the strided (w, h) passes,
 *                      workgroups of the z pass, workgroups of the larger strided pass.  No grid cap: one workgroup per tile.
 *                      ALQ_EUNSUPPORTED and out = -1 for dims alq_edt_sq refuses.
 *   alq_masked_dist_stats   d_out double [4] = over the elements i < n with d_mask[i] != 0: their number (exact), the sum of
 *                      sqrt(d_d2[i]), the maximum and the minimum of d_d2[i]; an empty mask gives 0, 0, -inf, +inf.  Fixed-order
 *                      reduction without float atomics: the same input gives the same bits on every run.
 *   alq_masked_select  d_out double [R], 1 <= R <= 8: d_out[r] = the h_ranks[r]-th smallest (0-based) of the masked values;
 *                      a rank at or above the masked count (which the host does not know) gives NaN.  h_ranks: host int64,
 *                      each >= 0.  The values must be non-negative doubles or +inf (radix selection on the bit pattern, which
 *                      orders those); NaN and negative values are outside the contract.  Integer atomics only: exact and
 *                      run-independent.  No host round trip inside a selection.
 * Both masked calls: 0 <= n < 2^31, d_work = alq_masked_work_bytes(n) bytes (0 for an n they refuse), 8-byte aligned like d_d2
 * and d_out.  alq_masked_geometry: out[2] = elements a workgroup takes per grid-stride step, workgroups of the launch for n.
 * ALQ_EINVAL: a null pointer, d_out == d_seg, a label above 255, a spacing that is 0, negative, infinite or NaN, R outside
 * 1 .. 8, a negative rank, a misaligned pointer, an axis below 1 (surface mask).  ALQ_EUNSUPPORTED: an axis outside
 * 1 .. alq_edt_max_axis() (distance transform), 2^31 voxels / elements or more.                                              */
int alq_surface_mask(alq_ctx *ctx, const uint8_t *d_seg, const int64_t dims[3], int label, uint8_t *d_out);
int alq_edt_max_axis(void);
size_t alq_edt_work_bytes(const int64_t dims[3]);
int alq_edt_geometry(const int64_t dims[3], int32_t out[4]);
int alq_edt_sq(alq_ctx *ctx, const uint8_t *d_feat, const int64_t dims[3], const double spacing2[3], double *d_out, void *d_work);
size_t alq_masked_work_bytes(int64_t n);
int alq_masked_geometry(int64_t n, int32_t out[2]);
int alq_masked_dist_stats(alq_ctx *ctx, const double *d_d2, const uint8_t *d_mask, int64_t n, double *d_out, void *d_work);
int alq_masked_select(alq_ctx *ctx, const double *d_d2, const uint8_t *d_mask, int64_t n, const int64_t *h_ranks, int R, double *d_out,
                      void *d_work);

/* ---- dense CRF on a two-class posterior map: exact mean-field inference (csrc/dcrf.hip) --------------------------------- */
/* Replaces: PW_analyze_results.DCRF_postprocess_2D (PW_analyze_results.py:539-591), pydensecrf's DenseCRF2D with 2 labels, a
 * smoothness kernel (create_pairwise_gaussian) and an appearance kernel (create_pairwise_bilateral), NORMALIZE_SYMMETRIC, Potts
 * compatibilities, `niter` mean-field iterations and the arg-max - with the two Gaussian filters evaluated exactly on a window
 * instead of on the library's permutohedral lattice.  dims = [S, H, W]: S independent slices, each plane contiguous in C order;
 * d_post, d_img float [S, H, W] (class-1 posteriors, image), both read-only.  Per slice, over the pixels raveled in C order:
 *   p = d_post, 0 read as 1e-10;  nl = -log p;  U = float32([1 - nl, nl])  (the reference's unary as it stands: label 0 gets
 *   1 + log p);  k(i, j) = exp(-|f_i - f_j|^2 / 2) with f = (row / sdims[0], column / sdims[1]) for the smoothness kernel and
 *   (row / sdims[0], column / sdims[1], img / schan) for the appearance kernel, on the window |d row| <= R_0, |d column| <= R_1,
 *   R = ceil(sdims sqrt(48 ln 2)) (6 and 29 for the defaults; the weight dropped is below 2^-24 of the peak), k(i, i) = 1;
 *   n_i = 1 / sqrt(sum_j k(i, j) + 1e-20) and (K~ Q)_i = n_i sum_j k(i, j) n_j Q_j over the same window, per kernel;
 *   Q = softmax(-U), then niter times Q = softmax(-U + compat_smooth K~_smooth Q + compat_app K~_app Q) over the two labels.
 * d_q1 float [S, H, W] = Q_1 after the last iteration, d_map uint8 [S, H, W] = [Q_1 > Q_0] (a tie gives 0); either may be
 * NULL, not both.  par NULL: the reference's values {1, 1}, {5, 5}, 1, 20, 30, 5.  d_work: alq_dcrf_work_bytes(dims) bytes
 * (20 per pixel; 0 for dims the call refuses), 4-byte aligned, disjoint from the outputs.  fp32 arithmetic, every sum in one
 * fixed order, no atomics: the same input gives the same bits.  2 + niter launches (one for niter = 0).
 * ALQ_EINVAL before any launch: a null required pointer, d_q1 and d_map both NULL, an axis below 1, 2^31 pixels or more, niter
 * outside [0, 64], a non-positive sdims or schan, a non-finite parameter.  ALQ_EUNSUPPORTED: a window radius above 31 or windows
 * whose staged tile exceeds the LDS of a compute unit (sdims above 5.37), more than 65535 slices.  Stream-ordered, no
 * synchronisation, no host read-back.                                                                                       */
typedef struct alq_dcrf_params {
    float sdims_smooth[2];     /* smoothness kernel: scale of the row and of the column coordinate */
    float sdims_app[2];        /* appearance kernel: the same */
    float schan;               /* appearance kernel: scale of the intensity */
    float compat_smooth, compat_app;
    int32_t niter;
} alq_dcrf_params;
size_t alq_dcrf_work_bytes(const int64_t dims[3]);
int alq_dcrf2d(alq_ctx *ctx, const float *d_post, const float *d_img, const int64_t dims[3], const alq_dcrf_params *par,
               float *d_q1, uint8_t *d_map, void *d_work);

/* ---- last-layer closed forms and the stochastic influence recursion (csrc/llfc.hip) -------------------------------- */
/* Replaces: NN.LLFC_grads / NN.LLFC_hess / NN.PW_LLFC_grads (NN.py:874-1029; duplicated in model_utils.py:137-292) and the
 * iteration of PW_NNAL.stoch_approx_IF (PW_NNAL.py:851-881).  u [d] = the input of the last fc layer (the model's feature
 * layer) of a sample, p [c] its posterior; a parameter vector holds W class-major (entry j*d + i) and then the c biases:
 * P = (d+1) c entries.  Features are taken as the caller hands them: any feature order, as long as pool and training
 * features share it.  d_feat [n, d] fp32 rows, d_post [c, n] fp32 (alq_forward's layouts), labels int32 [n].
 *   alq_llfc_grads     d_out [n, P] fp32, row n = (([j == y_n] - p_jn) u_n for j < c, [j == y_n] - p_jn): fp32 arithmetic
 *   alq_llfc_hess      d_H [P, P] fp64 of ONE sample: A (x) (u~ u~^T), u~ = (u, 1), A_jk = p_j (p_k - [j == k]); symmetric bit
 *                      for bit.  ALQ_EUNSUPPORTED when P * P * 8 exceeds alq_llfc_hess_max_bytes() (256 MiB): the recursion
 *                      below never forms the matrix
 *   alq_llfc_stoch_if  d_V [n_pool, P] fp32: V_0 = G (the gradients at d_pool_labels, each entry the fp64 product rounded
 *                      once), then for t < T with r = d_draws[t] (int32, clamped to [0, n_tr)):  V <- G + V + H_r V / scale,
 *                      done per column as c dot products and a rank-c update in fp64, V rounded to fp32 once per iteration.
 *                      path 1: columns stay in LDS over all T iterations (one launch; needs c <= 4 and c d 4 bytes within
 *                      the LDS of a CU, else ALQ_EUNSUPPORTED), path 2: V streams through HBM, two launches per iteration,
 *                      d_work = alq_llfc_if_work_bytes(n_pool, c) bytes (may be NULL on path 1), path 0: what
 *                      alq_llfc_if_path(d, c) names.  Both paths sum in one fixed order: the same bits, run after run.
 *                      n and n_pool <= 65535 per call (columns are independent: a larger pool is walked in slices).     */
int alq_llfc_grads(alq_ctx *ctx, const float *d_feat, const float *d_post, const int32_t *d_labels, int n, int d, int c,
                   float *d_out);
size_t alq_llfc_hess_max_bytes(void);
int alq_llfc_hess(alq_ctx *ctx, const float *d_feat_one, const float *d_post_one, int d, int c, double *d_H);
int alq_llfc_if_path(int d, int c);
size_t alq_llfc_if_work_bytes(int n_pool, int c);
int alq_llfc_stoch_if(alq_ctx *ctx, const float *d_pool_feat, const float *d_pool_post, const int32_t *d_pool_labels, int n_pool,
                      const float *d_tr_feat, const float *d_tr_post, int n_tr, const int32_t *d_draws, int T, double scale, int d,
                      int c, int path, float *d_V, void *d_work);

/* ---- A-optimal design of the `fi` query: the O(n) side of a Newton step (csrc/aopt.hip) ------------------------------- */
/* Replaces: the candidate-sized NumPy work of NNAL_tools._aopt_newton, this build's solver of the reference's query SDP at
 * lambda = 0 (NNAL_tools.py:612-659: min tr((sum_i q_i A_i)^-1) over the simplex).  The loop, the L x L and m x m algebra
 * (m = L(L+1)/2) and the step-size decisions stay on the host (DeviceSession.aopt_design); per Newton step the four launches
 * below move O(m^2) doubles and nothing of size n.  All arithmetic is fp64.  d_V [n, m]: the candidates' A_i in the orthonormal
 * symmetric basis; d_q, d_dq [n].  Supported: 1 <= L <= 8 and 1 <= n < 2^31 / m, else ALQ_EUNSUPPORTED.  h_* arrays must stay
 * unchanged until the stream has passed the call.  d_work: alq_aopt_work_bytes(n, L) bytes, shared by all launches of one solve.
 * Every sum is taken in one fixed order (tiles of alq_aopt_tile() candidates, a fixed grid for a given n, per-workgroup
 * partials folded in workgroup order, no atomics): the same inputs give the same bits on every run.  Candidates beyond n
 * are never read.  alq_aopt_max_workgroups(): the largest grid; beyond tile * max_workgroups candidates a workgroup walks several tiles.
 *   alq_aopt_svec        d_V[i, c] = A_i[a, b] for a == b, sqrt(2) A_i[a, b] for a < b; c walks the upper triangle row by row.
 *                        d_A [n, L, L] as alq_fisher writes it
 *   alq_aopt_stats       d_i = V_i . kvec,  r_i = (-d_i - mu / q_i) + (obj + n mu),  w_i = q_i^2 / mu,  u_i = R^T V_i (h_R [m, m] row
 *                        major).  d_out: the upper triangle, row by row, of  sum_i w_i u~_i u~_i^T  with u~_i = (u_i, r_i, 1)
 *                        [(m+2)(m+3)/2 doubles: G = sum w u u^T, h_r = sum w r u, h_1 = sum w u, s_r = sum w r, s_1 = sum w are
 *                        its blocks], then max_i d_i:  (m+2)(m+3)/2 + 1 doubles
 *   alq_aopt_direction   d_dq[i] = -(w_i r_i - sum_k w_i u_ik c_r[k]) + ratio (w_i - sum_k w_i u_ik c_1[k]);
 *                        d_out = (-sum_i r_i dq_i,  min over dq_i < 0 of -q_i / dq_i (+inf when none),  sum_i dq_i V_i [m])
 *   alq_aopt_linesearch  d_out[j] = sum_i log(q_i + h_alpha[j] dq_i) for j < J <= 64,  d_out[J] = sum_i log q_i
 *   alq_aopt_update      q <- q + alpha dq, then q <- q / sum(q);  d_out = (that sum, sum_i q_i V_i [m] of the normalised q)  */
int alq_aopt_tile(void);
int alq_aopt_max_workgroups(void);
size_t alq_aopt_work_bytes(int64_t n, int L);
int alq_aopt_svec(alq_ctx *ctx, const double *d_A, int64_t n, int L, double *d_V);
int alq_aopt_stats(alq_ctx *ctx, const double *d_V, const double *d_q, int64_t n, int m, const double *h_kvec,
                   const double *h_R, double mu, double obj, double *d_out, void *d_work);
int alq_aopt_direction(alq_ctx *ctx, const double *d_V, const double *d_q, int64_t n, int m, const double *h_kvec,
                       const double *h_R, const double *h_c_r, const double *h_c_1, double ratio, double mu, double obj,
                       double *d_dq, double *d_out, void *d_work);
int alq_aopt_linesearch(alq_ctx *ctx, const double *d_q, const double *d_dq, int64_t n, const double *h_alpha, int J,
                        double *d_out, void *d_work);
int alq_aopt_update(alq_ctx *ctx, double *d_q, const double *d_dq, const double *d_V, int64_t n, int m, double alpha,
                    double *d_out, void *d_work);

/* ---- fp64 accuracy reference on the device (csrc/ref64.hip; bench.py `accuracy`, tests) ------------------------------- */
/* One inverted decision of an fp64 evaluation.  layer = model layer index of a ReLU'd conv / conv_transpose / fc layer: the
 * ReLU decision of element `idx` of that layer's pre-activation of ONE sample ([vox, C] flattened; fc: the unit) is
 * inverted (passes although <= 0, cut although > 0); layer = index of a max-pool layer: element `idx` of the pool's INPUT is
 * lifted by `delta` before the window maximum is taken (a near-tie decided the other way).  layer < 0: unused slot.
 * In candidate lists `pad` is 0 for a ReLU unit, 1 for a pool window.                                                   */
typedef struct {
    int32_t layer;
    int32_t pad;
    int64_t idx;
    double delta;
} alq_flip_t;
/* fp64 evaluation of the scored path for N samples (rows d_rows of the fp32 pool d_x, or its first N rows when d_rows is
 * NULL): the reference's graph (conv / conv_transpose / max-pool / fc, 'con' skips; NN.py:258-340, NN_extended.py:366-601)
 * in double precision, one backward pass with the unit cotangent (+1, -1) on the two logits, and the per-layer sums
 * S[n][t] = sum of all entries of d(z0 - z1)/d(theta_t) - what NNAL_tools.shrink_gradient(., 'sum') (NNAL_tools.py:784-796)
 * divides by the layer's size.  h_dW / h_db: host arrays of DEVICE pointers to the fp64 weights / biases of the parameterised
 * layers, TF layouts as alq_model_set_weights EXCEPT fc: [out][in] with `in` in ACTIVATION-MEMORY order ([D, H, W, C]
 * flattened) of the layer's input.  d_flips: [N][flips_per_sample] decisions to invert per sample, or NULL.
 * cand_cap > 0: d_cand / d_cand_key / d_cand_count [N][cand_cap] / [N] receive every FRAGILE decision of a sample - a ReLU
 * input with |pre-activation| <= eps * (rms pre-activation of that layer and sample), key = that ratio; a pool window whose two
 * largest inputs lie within eps * (rms of the pool's input) of each other with a positive maximum, key = gap / rms, idx = the
 * runner-up, delta = the lift that makes it win - in no particular order; d_cand_count may exceed cand_cap (list truncated).
 * d_logits [N][2], d_S [N][L], d_rms [n_layers][N] (rms pre-activation / pool input per layer and sample; may be NULL).
 * Allocates its workspace per call and synchronises the stream: an accuracy tool, never on the scoring path.             */
int alq_ref64_scores(alq_ctx *ctx, const alq_layer_t *layers, int n_layers, const int32_t in_dims[4],
                     const double *const *h_dW, const double *const *h_db, const float *d_x, const int64_t *d_rows, int N,
                     const alq_flip_t *d_flips, int flips_per_sample, double eps, int cand_cap,
                     double *d_logits, double *d_S, double *d_rms, alq_flip_t *d_cand, double *d_cand_key, int32_t *d_cand_count);

/* ---- measurement hooks (bench.py only) -------------------------------------------------- */
/* Per-kernel-class HIP-event timing on the context's stream.  alq_prof_enable(ctx, 1) makes
 * every launch of an instrumented kernel class record start/stop events; on = k > 1 samples the
 * launches of every k-th alq_fisher pass only (the event pairs themselves cost a few percent);
 * alq_prof_read returns, for class `cls`, the accumulated milliseconds, launch count and
 * algorithmic FLOPs since the last alq_prof_reset (synchronises the stream).                 */
int alq_prof_enable(alq_ctx *ctx, int on);
int alq_prof_reset(alq_ctx *ctx);
int alq_prof_num_classes(void);
const char *alq_prof_class_name(int cls);
int alq_prof_read(alq_ctx *ctx, int cls, double *ms, int64_t *launches, double *flops);

/* Debug / test hook: copies an internal tensor of the last alq_forward / alq_fisher call into a
 * dense device buffer.  what: 0 = activation of layer `layer_idx` [N, vox, C], 1 = its cotangent
 * (after the ReLU mask), 2 = channel-sum field of the layer's INPUT [N, vox_in], 3 = channel-sum
 * field of its masked cotangent [N, vox_out], 4 = the unit-cotangent layer sums S [N, L] (as
 * float; layer_idx ignored), 5 = the fused fc head's logit-difference partials [N, tiles * 4] (one per
 * (tile, wave) of the last conv's launch); of a wide fc layer (streaming GEMM), as raw bytes in 4-byte words: 6 / 7 = the packed
 * bf16 triples / fp16 pairs of its forward Gemm, 8 / 9 = of its backward Gemm, 10 = 4 words: the fp16 scale exponents of the
 * forward and the backward plan and the bits of the layer's fp64 L1 bound (N ignored); after a Fisher pass: 11 = channel-sum field of
 * the layer's OUTPUT [N, vox_out], 12 = the sign field of the rows its output lies in, as raw bytes in 4-byte words ([N, vox_out, cs / 4]
 * bytes, cs = channels of the allocation: the layer's own bytes are the C / 4 from byte c0 / 4 of a voxel; bit k of a byte = (channel
 * 4 b + k > 0)), 13 = a pool layer's arg-max field as raw bytes in 4-byte words ([N, vox_out, C] window indices), 14 = the sign bytes a
 * two-class fc head (layer_idx) keeps of its input, as raw bytes in 4-byte words ([N, F / 4] bytes in activation-memory order: bit k
 * of byte j = (element 4 j + k > 0), bits 5 - 7 clear, bit 4 clear unless ALQ_NO_FLIPFIX=1 left a mark; ALQ_EUNSUPPORTED where the
 * layer has no such field or the last pass was no Fisher pass).
 * The fp16-pair scales of the last pass, as the floats whose bits the launches read: 15 = the derived per-patch bounds on every layer's
 * output [layers, N] (layer_idx ignored; ALQ_EUNSUPPORTED where the pass derived none), 16 = the measured per-patch maxima of the
 * output of layer_idx [N] (ALQ_EUNSUPPORTED where the pass did not ask that layer's launch for them), 17 = the measured per-patch maxima
 * of the network input [N] (layer_idx ignored; ALQ_EUNSUPPORTED unless the pass scaled the first launch by them), 18 = the static
 * bounds on every layer's output cotangent in the backward sweep of the last Fisher pass [layers] (layer_idx and N ignored; -1 =
 * unknown; ALQ_EUNSUPPORTED where the last call was no Fisher pass).
 * *elems_out receives the element count.  Tests only.  */
int alq_model_debug_copy(alq_model *m, int layer_idx, int what, int N, float *d_out,
                         int64_t *elems_out);
/* Tests only: the two kernels behind the derived bounds on caller buffers (device pointers, the context's stream).
 * alq_debug_rowmax_abs: d_out[n] = the bits of max_k |d_x[n * K + k]| (a NaN is dropped: the maximum of the rest).
 * alq_debug_fwd_bounds: d_bound_all[k * stride + p] = the bits of bound_k(p) for k < nl <= 16 and p < N <= stride, where
 * bound_0 = amax0 (from_input: amax0 * L[0] + B[0]) and bound_k = max(bound_{k-1}, bound_{src2[k]} if src2[k] >= 0) * L[k] + B[k];
 * L, B and src2 are host arrays of nl entries, src2[k] in [-1, k).                                                          */
int alq_debug_rowmax_abs(alq_ctx *ctx, const float *d_x, int N, int64_t K, uint32_t *d_out);
int alq_debug_fwd_bounds(alq_ctx *ctx, const uint32_t *d_amax0, int N, int stride, const float *L, const float *B,
                         const int32_t *src2, int nl, int from_input, uint32_t *d_bound_all);

/* Diagnostic builds only (-DALQ_STAMPS): device buffer of 8 uint64 per workgroup that receives the
 * per-phase shader-clock ticks of the pipelined GEMM kernel's next launches; NULL switches it off.
 * A no-op in the product build.                                                               */
int alq_debug_set_stamp_buffer(void *d_buf);
/* Timing-experiment knobs (tests / profiling only; results may be wrong while a knob is set):
 * key 0 = repeat the MFMA phase n extra times, 1 = flag bits (1 no stores, 2 no loads, 4 no sum
 * MFMAs, 8 no sum stores), 2 = no epilogue fusion in backward GEMMs, 3 = none in forward GEMMs,
 * 4 = use the fp32-MFMA GEMM kernel instead of the bf16x3 split kernel, 7 = first conv and the pool behind
 * it as separate launches, 8 = the first conv + pool kernel on its narrow tile with per-voxel sum / sign
 * stores everywhere (same bits; ALQ_DCP_NARROW at model creation), 9 = at most that many workgroups in
 * the plane-sweep launch of csrc/e3d.hip (same bits; lets a handful of patches make multi-patch streams),
 * 10 = the same cap for the 7-k-step backward launch of csrc/c3d.hip (same bits).                          */
int alq_debug_set(int key, int value);
/* What the last pass of a model ran on (tests / bench reporting).  what = 0: 1 when the matrix cores of the context's device
 * keep fp16 subnormal operands (probed once; the one-accumulator form of the plane-sweep engine needs it), 1: 1 when the last
 * forward pass ran the conv under the two-class head on the plane-sweep engine (csrc/c3d.hip; replaces the tf.nn.conv3d call
 * site NN_extended.py:416-426 for that layer), 2: the same for the last backward pass, 3: 1 when that engine accumulates the
 * three piece products in one accumulator, 5: the number of marked 4-channel groups that did not fit their list segment (a quarter of a patch,
 * 128 slots) since the model was created - 0 on every input the tests and the bench use; none is dropped: an overflowing
 * segment is drained by the sweep path of the fix-up kernel (synchronises the stream).
 * 6: 1 when the last forward pass ran a launch on the fp16-pair split with derived input bounds (default; ALQ_NO_F16_DERIVED=1 off).
 * 7 / 8: conv_transpose launches of the last forward / backward pass on the row-sweep engine (csrc/t3d.hip), 9: 1 when the last
 * backward pass ran enc2's backward fused with both pool backward steps (csrc/e3d.hip), 10: 1 when the last forward pass ran
 * dec1 on the plane-sweep kernel of csrc/d3d.hip, 11: the same for its backward-data launch, 12: 1 when the last forward pass
 * ran enc2 and the max-pool behind it as one launch (csrc/f3d.hip), 13: which form of the head conv's backward kernel the last backward
 * pass ran (csrc/c3d.hip): 7 = the 27 taps packed into 7 k-steps (default), 8 / 4 = the 9-k-step kernel (ALQ_C3D_BWD_ROWS), 0 = none.
 * 14: the number of weight elements that went through the HOST packers since the model was created (alq_model_set_weights, the
 * per-layer fall-back of alq_model_set_weights_device and the lazy forms behind the debug knobs); saturates at 2^31 - 1.
 * 15: 1 when the last general backward sweep ran the fused layer-sum kernels of csrc/lsum.hip (alq_class_layer_sums), 0 after
 * alq_param_grads / alq_grad_sqnorms.
 * 16: form of the first conv + pool kernel (csrc/direct.hip) in the last forward pass: 0 = it did not run, 1 / 2 = narrow tile
 * (8 x 16 x 16 voxels) with scalar / 16-byte row loads, 4 / 5 = the same on the wide tile (8 x 8 x 32), 6 = wide tile on whole-tile
 * volumes with 16-byte channel-sum and sign-byte stores.
 * 17: form of the fused enc2 backward launch (csrc/e3d.hip) in the last backward pass: 0 = it did not run, 2 = the z plane sweep
 * (default), 1 = the row sweep (ALQ_E3D_ROWS=1 at model creation; same bits).
 * 19: waves per SIMD of the head conv's backward kernel (csrc/c3d.hip) in the last backward pass: 0 = it did not run, 2 = the 7-k-step
 * kernel on 512 threads, four rows per wave (default), 1 = one wave per SIMD (ALQ_C3D_BWD_WAVES=1 at model creation - same bits -
 * and the 9-k-step forms).  (18 stays unused: callers have relied on it being refused.)
 * 20: workgroups of that launch (0 = it did not run): min(patches, 256) unless alq_debug_set(10, g) capped it (tests).
 * The backward indices 2, 8, 9, 11, 13, 17, 19 and 20 name launches of the Fisher pass only: all of them are 0 after a general backward
 * sweep (alq_param_grads, alq_grad_sqnorms, alq_class_layer_sums, alq_diag_fisher, the loss entry points) and after alq_hess_vecp,
 * whatever an earlier Fisher pass on the same model ran.
 * Returns the answer or a negative error code (ALQ_EINVAL for 4 and 18, which are unused, and for anything outside 0 .. 20).  */
enum {
    ALQ_INFO_SUBNORMALS_OK = 0,
    ALQ_INFO_C3D_FWD = 1,
    ALQ_INFO_C3D_BWD = 2,
    ALQ_INFO_C3D_ONE_ACC = 3,
    ALQ_INFO_FLIP_OVERFLOW = 5,
    ALQ_INFO_F16_DERIVED = 6,
    ALQ_INFO_T3D_FWD = 7,
    ALQ_INFO_T3D_BWD = 8,
    ALQ_INFO_E3D_BWD = 9,
    ALQ_INFO_D3D_FWD = 10,
    ALQ_INFO_D3D_BWD = 11,
    ALQ_INFO_F3D_FWD = 12,
    ALQ_INFO_C3D_BWD_FORM = 13,
    ALQ_INFO_HOST_PACK_ELEMS = 14,
    ALQ_INFO_LSUM = 15,
    ALQ_INFO_DCP_FORM = 16,
    ALQ_INFO_E3D_BWD_FORM = 17,
    ALQ_INFO_C3D_BWD_WAVES = 19,
    ALQ_INFO_C3D_BWD_GRID = 20
};
int alq_model_engine_info(alq_model *m, int what);

/* Synthetic patch generator: counter-based RNG keyed (seed, patch_id, element), standard
 * normal, written to d_out [n, elems_per_patch] for patch ids first_id .. first_id+n-1
 * (shards are reproducible whatever the sharding).                    */
int alq_synth_patches(alq_ctx *ctx, uint64_t seed, int64_t first_id, int64_t n,
                      int64_t elems_per_patch, float *d_out);

/* ---- resident volumes and the batches cut from them (csrc/volbatch.hip) ---------------------------------------------------- */
/* Replaces: the per-sample, per-plane, per-modality loop of datasets/utils.prepare_batch_BrVol and the strided slice reads
 * `img[:, :, s]` behind it.  A subject is uploaded once, packed once, and a batch is one launch (per 64 samples).
 *
 * alq_vol_pack: m device arrays [H, W, Z] in C order (z fastest) of `src_type` -> d_out [Z, H, W, m] floats; dims = {H, W, Z}.
 * double rounds to nearest even once, the integer types are exact.  alq_mask_pack: a class-id volume of bytes [H, W, Z] ->
 * [Z, H, W] (255: no class).  ALQ_EINVAL: a null pointer, an axis below 1, another src_type; ALQ_EUNSUPPORTED: m above 8.   */
enum { ALQ_SRC_F32 = 0, ALQ_SRC_F64 = 1, ALQ_SRC_I16 = 2, ALQ_SRC_U8 = 3 };
int alq_vol_pack(alq_ctx *ctx, const void *const *d_src, int m, int src_type, const int32_t *dims, float *d_out);
int alq_mask_pack(alq_ctx *ctx, const uint8_t *d_src, const int32_t *dims, uint8_t *d_out);
/* alq_slice_batch: b windows of crop = {z, h, w} voxels out of nvol packed subjects.  h_vols / h_masks: HOST arrays [nvol] of the
 * device pointers alq_vol_pack / alq_mask_pack filled (a mask may be NULL for a subject no labelled sample names), h_dims host
 * [nvol][3] = {H, W, Z} of each, h_desc host [b][5] = (subject, zc, h0, w0, labelled 0 / 1).  Outputs:
 *   d_X [b, z, h, w, m] floats, X[i, jz, r, s, j] = vol[zc - z/2 + jz, h0 + r, w0 + s, j];
 *   d_lab [b, z, h, w] int32: the mask byte, or -1 where the sample is unlabelled or the byte is >= C;
 *   d_counts int64 [C + 1]: the voxels of every class, the -1 voxels last (zeroed by the call).
 * Every descriptor is checked on the host before anything is launched or written (alq_slice_batch_check, the same check without
 * a device): subject in range, 0 <= zc - z/2, zc - z/2 + z <= Z, 0 <= h0, h0 + h <= H, 0 <= w0, w0 + w <= W, the flag 0 or 1,
 * 1 <= C <= 254, a crop axis below 1: ALQ_EINVAL.  Stream-ordered, no synchronisation; the host arrays are read before return.
 * alq_slice_batch_trip_rows: the output rows (i, jz, r) one sweep of the capped grid covers; alq_slice_batch_launch_samples: the
 * samples of one launch (for tests: a case asserts from these that it passes them).                                             */
int alq_slice_batch_check(const int32_t *h_dims, int nvol, const int32_t *h_desc, int b, const int32_t *crop, int C);
int alq_slice_batch(alq_ctx *ctx, const float *const *h_vols, const uint8_t *const *h_masks, const int32_t *h_dims, int nvol, int m,
                    const int32_t *h_desc, int b, const int32_t *crop, int C, float *d_X, int32_t *d_lab, int64_t *d_counts);
int64_t alq_slice_batch_trip_rows(void);
int alq_slice_batch_launch_samples(void);

/* ---- whole-volume inference of a dense model: tiles, blended on the device (csrc/tile.hip) ----------------------------------- */
/* No reference counterpart (the reference builds one model per image size, eval_utils.models_dict_for_different_sizes); the NumPy
 * statement of every function below is nnal_amd/tiled.py, and the device equals it bit for bit.
 *
 * The lattice, order Z, H, W.  Along an axis of length D with tile t and stride s (1 <= s <= t): D <= t gives one tile at origin 0,
 * which overhangs the volume by t - D at the high end; otherwise there are ceil((D - t) / s) + 1 tiles at min(i s, D - t) - the last
 * one is clamped so that it ends with the volume.  Tile (iz, ih, iw) has the index (iz nH + ih) nW + iw.  The three lattice functions
 * are host arithmetic and make no device call.
 *   alq_tile_lattice_check  ALQ_EINVAL: null, an axis or a tile below 1, a stride below 1 or above the tile.
 *   alq_tile_count          the tiles per axis into counts (may be NULL); returns their product, or the check's error.
 *   alq_tile_origin         the first voxel of tile idx; ALQ_EINVAL: idx outside 0 .. count - 1, null origin.
 *
 * alq_tile_gather: d_vol is a packed volume [Z, H, W, m] of floats (alq_vol_pack); writes d_X [n, tz, th, tw, m], the tiles
 * first .. first + n - 1.  Voxels outside the volume - they occur only on an axis with D < t - are `fill`.  1 <= m <= 8.
 *
 * alq_tile_blend: d_post [c, n V] in class-major planes as alq_forward writes them for a dense model, V = tz th tw, sample j V + v
 * is voxel v of tile first + j; d_wz [tz], d_wh [th], d_ww [tw] the window tables; d_acc [c + 1, Z, H, W], zeroed by the caller
 * before the first call.  For every voxel and every tile of the call that covers it, in ascending tile index, with (lz, lh, lw) the
 * voxel's place in the tile and every operation rounded to fp32 on its own:
 *     w = (wz[lz] wh[lh]) ww[lw];    acc[k] += w p_k, k = 0 .. c - 1;    acc[c] += w.
 * A voxel has one writer and its sum runs in tile order whatever the calls' ranges: calls over consecutive ranges of tiles leave
 * the bytes of one call over all tiles.  The overhang of a tile is never written.  2 <= c <= 8.
 * alq_tile_blend_trip_voxels: the voxels one sweep of the capped grid covers (for tests: a case asserts from it that the bounding
 * box of its call passes them).
 *
 * alq_tile_finalize: dims = {Z, H, W}; q_k = acc[k] / acc[c], correctly rounded, into d_post_out [c, ...] (may be NULL); the first
 * maximum of q over k into d_label bytes (may be NULL).  hwz = 0: both in [Z, H, W] order; hwz = 1: [H, W, Z] with z fastest, the
 * layout alq_cc_*, alq_surface_mask and alq_confusion_counts read.  2 <= c <= 8.
 *
 * All three are stream-ordered with no synchronisation.  Refused before any launch - ALQ_EINVAL: a null pointer, a bad lattice,
 * first < 0, n < 1, first + n beyond the tile count, m < 1, hwz outside {0, 1}, a misaligned pointer; ALQ_EUNSUPPORTED: m or c out
 * of range, a volume or a call's tiles of 2^31 voxels (elements, for the gather) or more.                                          */
typedef struct { int32_t dims[3], tile[3], stride[3]; } alq_tile_lattice_t;   /* order Z, H, W */
int alq_tile_lattice_check(const alq_tile_lattice_t *lat);
int64_t alq_tile_count(const alq_tile_lattice_t *lat, int32_t counts[3]);
int alq_tile_origin(const alq_tile_lattice_t *lat, int64_t idx, int32_t origin[3]);
int alq_tile_gather(alq_ctx *ctx, const float *d_vol, int m, const alq_tile_lattice_t *lat, int64_t first, int64_t n, float fill, float *d_X);
int alq_tile_blend(alq_ctx *ctx, const float *d_post, int c, const alq_tile_lattice_t *lat, int64_t first, int64_t n, const float *d_wz,
                   const float *d_wh, const float *d_ww, float *d_acc);
int64_t alq_tile_blend_trip_voxels(void);
int alq_tile_finalize(alq_ctx *ctx, const float *d_acc, int c, const int32_t dims[3], int hwz, float *d_post_out, uint8_t *d_label);

/* ---- SLIC super-pixel over-segmentation of a resident subject (csrc/slic.hip) ---------------------------------------------- */
/* Makes the over-segmentation alq_segment_min reads, where the reference calls skimage.segmentation.slic (PW_AL.py:2).  NOT
 * skimage: there is no reference counterpart to match, the algorithm is defined by its NumPy statement nnal_amd/slic.py (a gSLIC
 * per axial slice on values quantised to 16 bits, integer cluster sums, then enforced 4-connectivity), and the device equals that
 * statement byte for byte whatever order its workgroups run in.  slic.py's docstring is the full definition; in short:
 *   d_vol   packed subject [Z, H, W, m] floats (alq_vol_pack), d_mask packed bytes [Z, H, W] or NULL: byte 255 = out (the NO_CLASS
 *           byte of alq_mask_pack), any other byte = in.  A pixel with a non-finite value in any channel is out as well.
 *   dims    {H, W, S}, S = Z slices.  lo, scale: HOST arrays [m]; q_c = clamp(rint((double(v) - lo[c]) * scale[c]), 0, 65535).
 *   gh, gw  cells per slice, 1 <= gh <= H, 1 <= gw <= W; w the spatial weight of d = sum_c (q_c - mu_c)^2 + w ((y - cy)^2 + (x - cx)^2);
 *           T iterations of assign + update (0: the home cells); min_size: a cluster's largest component is kept only from that
 *           size on (0: always), every other component is adopted by a kept region it touches or merged with its fellow orphans.
 *   d_labels int32, [H, W, S] with hwz = 1 (what alq_segment_min reads), [S, H, W] with hwz = 0: 0 on out pixels, else 1 .. n_z in
 *           the order of the regions' first pixels; d_nlabels int32 [S] = n_z.
 *   d_work  alq_slic_work_bytes(dims, m, gh, gw) bytes (0 for arguments alq_slic refuses), 8-byte aligned: centres, cluster keys,
 *           four int32 volumes and the uint16 pixels.
 * One launch sequence for all slices: 2 + 2 T + 10 launches, no host round trip and no copy back - the adoption rounds loop inside a
 * launch on a flag in LDS.  Measured (MI355X, 256 x 256 x 128, m = 1, a 32 x 32 grid, T = 10; DESIGN.md section 7 has the table):
 * 4.68 ms the call, 0.31 ms an iteration - 24 times a device copy of the iteration's bytes, bound by latency, not by bytes -
 * against 2.4 s for the statement on 16 host threads.  Stream-ordered, no synchronisation.  Refused before any launch - ALQ_EINVAL: a null pointer (d_mask may
 * be NULL), an axis, m, gh or gw below 1, gh > H, gw > W, w negative or not finite, T or min_size below 0, hwz outside {0, 1}, a
 * lo / scale that is not finite, a misaligned pointer; ALQ_EUNSUPPORTED: m above 8, 2^31 pixels or more.
 * alq_slic_geometry (for tests: a case asserts from it that it is in the regime it names): out[0] = (slice, tile) pairs of the
 * assign launch, out[1] = its workgroups, out[2] = clusters one update workgroup reduces per sweep, out[3] = update workgroups,
 * out[4] = workgroups of the per-slice launches (one slice each per sweep), out[5] = the cap on every grid (8 per CU; the
 * environment variable ALQ_SLIC_MAX_GROUPS overrides it, same bytes for every value), out[6] = workgroups of the per-pixel
 * launches (256 pixels each per sweep), out[7] = the tile side.  A capped grid strides: workgroup b takes items b, b + grid, ...   */
size_t alq_slic_work_bytes(const int64_t dims[3], int m, int gh, int gw);
int alq_slic_geometry(alq_ctx *ctx, const int64_t dims[3], int m, int gh, int gw, int64_t out[8]);
int alq_slic(alq_ctx *ctx, const float *d_vol, const uint8_t *d_mask, const int64_t dims[3], int m, const double *lo, const double *scale, int gh,
             int gw, double w, int T, int min_size, int hwz, int32_t *d_labels, int32_t *d_nlabels, void *d_work);

#ifdef __cplusplus
}
#endif
#endif /* ALQ_H */
