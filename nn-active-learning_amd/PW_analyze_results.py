"""Test-set evaluation of the patch-wise AL loop (reference: PW_analyze_results.py): the confusion statistics and F1 scores
(`get_preds_stats`, `get_Fmeasure`, `F1_scores`), the query files of a method (`get_queries`), dense slice / volume
evaluation (`full_slice_eval`, `full_model_eval`) and the learning curve of a method over its stored weights
(`eval_MultimgAL`, which writes `<method>/test_scores.txt`).  Signatures as in the reference.

The three metric functions are host NumPy, the reference's operations in its order.  The evaluations that walk many voxels
keep the predictions on the device: `eval_counts_device` feeds every chunk's prediction tensor to alq_eval_counts, which adds
to six int64 totals in HBM (and scatters the predictions into a uint8 volume for full_model_eval); 48 bytes come back.
full_model_eval(..., post_process=True) applies the reference's post-processing (post_processing.py: largest connected
component, hole filling) to that volume where it lies (alq_cc_keep_largest, alq_fill_holes) before scoring and saving it.
The dense-CRF post-processing (`DCRF_postprocess_2D`, `full_model_pred_DCRF`) runs on the device as well: alq_dcrf2d computes
the reference's CRF model with exact windowed Gaussian filters (nnal_amd.dcrf states the model and is its host oracle) on the
posteriors where posteriors_device left them.

Not mirrored: `grid_based_F1` (patch_utils.generate_grid_samples is outside this package), `full_test_slice_DCRF` and
`DCRF_postprocess_3D`, the plotting helpers (`visualize_eval_metrics`, ...) and the super-pixel helpers: they need skimage /
matplotlib and sit beside the scored path, not on it."""
import os

import numpy as np

from . import PW_NN, nrrd_io, patch_utils


def get_queries(expr, method_name):
    """PW_analyze_results.py:29-50: the queries of every iteration of a method, in numeric order of the file names
    (`queries/<iter>`), each as np.int32(np.loadtxt(file))."""
    Q_dir = os.path.join(expr.root_dir, method_name, 'queries')
    Q_files = os.listdir(Q_dir)
    file_inds = [int(Q_files[i].split('.')[0]) for i in range(len(Q_files))]
    return [np.int32(np.loadtxt(os.path.join(Q_dir, Q_files[ind]))) for ind in np.argsort(file_inds)]


def get_preds_stats(preds, mask):
    """PW_analyze_results.py:234-258: (P, N, TP, FP, TN, FN) of predictions against labels of the same shape, six Python
    floats.  A NaN (or negative) label satisfies neither `mask > 0` nor `mask == 0` and counts nowhere."""
    P = float(np.sum(mask > 0))
    N = float(np.sum(mask == 0))
    TP = float(np.sum(np.logical_and(preds > 0, mask > 0)))
    FP = float(np.sum(np.logical_and(preds > 0, mask == 0)))
    TN = float(np.sum(np.logical_and(preds == 0, mask == 0)))
    FN = float(np.sum(np.logical_and(preds == 0, mask > 0)))
    return P, N, TP, FP, TN, FN


def get_Fmeasure(preds, mask):
    """PW_analyze_results.py:261-289: F measure of one prediction array, or of dicts path -> array summed over their keys.
    NumPy integer sums, so a zero denominator gives nan / inf with a warning where the float code of F1_scores raises."""
    P = 0
    TP = 0
    TPFP = 0
    if isinstance(preds, dict):
        for img_path in list(preds.keys()):
            ipreds = preds[img_path]
            imask = np.array(mask[img_path])
            P += np.sum(imask > 0)
            TP += np.sum(np.logical_and(ipreds > 0, imask > 0))
            TPFP += np.sum(ipreds > 0)
    else:
        P += np.sum(mask > 0)
        TP += np.sum(np.logical_and(preds > 0, mask > 0))
        TPFP += np.sum(preds > 0)
    Pr = TP / TPFP
    Rc = TP / P
    return 2 / (1 / Pr + 1 / Rc)


def F1_scores(preds, labels):
    """PW_analyze_results.py:291-295 (Python floats: ZeroDivisionError without predicted positives or without positives)."""
    P, N, TP, FP, TN, FN = get_preds_stats(preds, labels)
    Pr = TP / (TP + FP)
    Rc = TP / P
    return 2 * Pr * Rc / (Pr + Rc)


def _f1_or_zero(P, TP, FP):
    """2 / (1/Pr + 1/Rc) as PW_AL.py:669-675 / PW_analyze_results.py:652-654 write it.  Deviation: where the reference's
    float divisions raise ZeroDivisionError (no predicted positives, or no positives at all) the score is 0, its own
    `Pr > 0 and Rc > 0` fallback - a fresh model that predicts one class must not abort a learning curve."""
    if TP + FP == 0 or P == 0:
        return 0
    Pr = TP / (TP + FP)
    Rc = TP / P
    if Pr > 0 and Rc > 0:
        return 2. / (1 / Pr + 1 / Rc)
    return 0


def _device_labels(sess, mask):
    """The mask volume / label vector as a contiguous float32 or float64 device tensor (a device tensor passes through)."""
    torch = sess.torch
    if isinstance(mask, torch.Tensor):
        return mask
    arr = np.asarray(mask)
    if arr.dtype != np.float32:
        arr = arr.astype(np.float64)
    return sess.to_device(arr, torch.float32 if arr.dtype == np.float32 else torch.float64)


def eval_counts_device(model, sess, img_dat, inds, patch_shape, batch_size, stats, mask, seg=None, _vols=None, _counts=None,
                       _preds=None):
    """(Not a reference function.)  get_preds_stats(batch_eval(..., 'prediction')[0], labels) without the predictions leaving
    the device: walks PW_NN._eval_passes - batch_eval's gather, statistics and passes - and hands every chunk's prediction
    tensor to alq_eval_counts.  `mask`: the subject's UN-padded 3-D mask volume (the label of inds[i] is mask.ravel()[inds[i]])
    or a 1-D label vector aligned with `inds` (gen_multimg_inds' labels); array or device tensor, NaN = counted nowhere.
    `seg` (volume form only): uint8 device tensor of the mask's size, seg[inds[i]] = prediction i.
    Returns (P, N, TP, FP, TN, FN) as Python floats after ONE copy of 48 bytes.
    `_counts`: an int64 device tensor [6] to add to instead - nothing is copied back and None is returned; `_preds`: an int64
    device tensor [len(inds)] that receives the predictions (test_eval's second return value)."""
    torch = sess.torch
    inds = np.ascontiguousarray(np.asarray(inds, dtype=np.int64))
    lab = _device_labels(sess, mask)
    volume = lab.dim() == 3
    if not volume and (lab.dim() != 1 or int(lab.numel()) != len(inds)):
        raise ValueError('`mask` must be the 3-D mask volume or one label per index (%d indices, labels %r)'
                         % (len(inds), tuple(lab.shape)))
    if seg is not None and not volume:
        raise ValueError('`seg` needs the mask volume form')
    flat = lab.reshape(-1)
    counts = _counts if _counts is not None else sess.to_device(np.zeros(6, dtype=np.int64), torch.int64)
    for a, b, _, pred, _ in PW_NN._eval_passes(model, sess, img_dat, inds, patch_shape, batch_size, stats, (1., False, 0), True,
                                               False, _vols, 0):
        if volume:
            sess.eval_counts(pred, sess.to_device(inds[a:b], torch.int64), flat, counts, seg)
        else:
            sess.eval_counts(pred, None, flat[a:b], counts, None)
        if _preds is not None:
            _preds[a:b] = pred
    if _counts is not None:
        return None
    return tuple(float(v) for v in counts.cpu().numpy())


def _padded_volumes(img_paths, patch_shape):
    """batch_eval's image argument (PW_NN.py:429-444): paths are read and zero-padded by the patch radii, arrays are taken
    as already padded.  Returns (padded arrays, un-padded shape)."""
    rads = patch_utils.patch_radii(patch_shape)
    if isinstance(img_paths[0], np.ndarray):
        vols = [np.asarray(v) for v in img_paths]
    else:
        vols = [np.pad(nrrd_io.read(p)[0], ((rads[0], rads[0]), (rads[1], rads[1]), (rads[2], rads[2])), 'constant')
                for p in img_paths]
    shape = tuple(int(vols[0].shape[a]) - 2 * rads[a] for a in range(3))
    return vols, shape


def _slice_inds_3D(img_shape, ind):
    """PW_analyze_results.py:687-706: the raveled 3-D indices of every voxel of slice `ind`, in the order of the slice's own
    raveled 2-D indices."""
    inds_2D = np.arange(0, int(np.prod(img_shape[:2])))
    multinds_2D = np.unravel_index(inds_2D, img_shape[:2])
    extra_inds = np.ones(len(inds_2D), dtype=int) * ind
    return multinds_2D, np.ravel_multi_index(multinds_2D + (extra_inds,), img_shape)


def full_slice_eval(model, sess, img_paths, slice_inds, patch_shape, ntb, stats, varname='prediction'):
    """PW_analyze_results.py:673-724: `varname` of every voxel of the slices `slice_inds` as a float64 [x, y, z] volume (zero
    elsewhere).  `img_paths`: paths or already padded arrays, as batch_eval accepts; the volumes are uploaded once for all
    slices."""
    vols, img_shape = _padded_volumes(img_paths, patch_shape)
    dv = patch_utils.DeviceVolumes(sess, vols)
    slice_evals = np.zeros(img_shape)
    for ind in slice_inds:
        multinds_2D, inds_3D = _slice_inds_3D(img_shape, ind)
        evals = PW_NN.batch_eval(model, sess, vols, inds_3D, patch_shape, ntb, stats, varname, _vols=dv)[0]
        eval_map = np.zeros(img_shape[:2])
        eval_map[multinds_2D] = evals
        slice_evals[:, :, ind] = eval_map
    return slice_evals


def full_model_eval(expr, model, sess, img_path, mask_path, slice_inds, save_dir=None, post_process=False):
    """PW_analyze_results.py:594-670: predictions of every voxel of the slices `slice_inds`, their F1 against the mask over
    those slices and, with `save_dir`, `segs.nrrd` (uint8) and `F1_socre.txt` (the reference's spelling).  Returns
    (preds [x, y, z] float64, F1).

    The reference's call `full_slice_eval(model, img_path, [ind], 'axial', ...)` (:616-624) passes its arguments in an order
    that cannot run; the evident intent is restated: slice by slice, expr.pars['patch_shape'], ['ntb'], ['stats'], all the
    modalities of `img_path` (one path / padded array, or a list of them).  Here the slices go through the device path: the
    predictions are scattered into a uint8 volume in HBM and counted against the resident mask by alq_eval_counts; one
    volume of bytes and 48 bytes of counts come back.  F1 is F1_scores' expression 2 Pr Rc / (Pr + Rc) on those counts, so
    that it equals F1_scores(preds[:, :, slice_inds], mask[:, :, slice_inds]) bit for bit (the reference's line :654 writes
    the same number as 2 / (1/Pr + 1/Rc), which may differ in the last place), and 0 where the reference's float divisions
    would raise (no predicted positives, no true positives, or no positives at all).

    `post_process` (eval_utils.get_full_segs' switch; not an argument of the reference's full_model_eval): the uint8 volume is
    post-processed on the device before it comes back - the largest 26-connected component outside voxel 0's
    (alq_cc_keep_largest; an all-zero volume when there is none), then the enclosed cavities filled (alq_fill_holes) - and
    the processed volume is what is returned, scored (alq_eval_counts on its voxels of the same slices) and saved; the
    unprocessed one goes to `segs_raw.nrrd` / `F1_socre_raw.txt`."""
    torch = sess.torch
    if save_dir:
        if not os.path.exists(save_dir):
            os.mkdir(save_dir)
    mask = mask_path if isinstance(mask_path, np.ndarray) else nrrd_io.read(mask_path)[0]
    img_paths = [img_path] if isinstance(img_path, (str, np.ndarray)) else list(img_path)
    patch_shape = expr.pars['patch_shape']
    vols, img_shape = _padded_volumes(img_paths, patch_shape)
    if tuple(mask.shape) != img_shape:
        raise ValueError('mask %r and image %r differ in shape' % (tuple(mask.shape), img_shape))
    dv = patch_utils.DeviceVolumes(sess, vols)
    lab = _device_labels(sess, mask)
    seg = sess.to_device(np.zeros(int(mask.size), dtype=np.uint8), torch.uint8)
    counts = sess.to_device(np.zeros(6, dtype=np.int64), torch.int64)
    for ind in slice_inds:
        _, inds_3D = _slice_inds_3D(img_shape, ind)
        eval_counts_device(model, sess, vols, inds_3D, patch_shape, expr.pars['ntb'], expr.pars['stats'], lab, seg=seg,
                           _vols=dv, _counts=counts)
    F1 = _f1_from_counts(counts)
    if post_process:
        if save_dir:
            nrrd_io.write(os.path.join(save_dir, 'segs_raw.nrrd'), np.uint8(seg.cpu().numpy().reshape(img_shape)))
            np.savetxt(os.path.join(save_dir, 'F1_socre_raw.txt'), [F1])
        seg, _ = sess.cc_keep_largest(seg, img_shape, connectivity=26, skip_origin=True, out=seg)
        seg, _ = sess.fill_holes(seg, img_shape, out=seg)
        inds = sess.to_device(np.concatenate([_slice_inds_3D(img_shape, ind)[1] for ind in slice_inds]), torch.int64)
        counts = sess.to_device(np.zeros(6, dtype=np.int64), torch.int64)
        sess.eval_counts(seg.reshape(-1)[inds].to(torch.int64), inds, lab.reshape(-1), counts, None)
        F1 = _f1_from_counts(counts)
    segs = seg.cpu().numpy().reshape(img_shape)
    print('\n F1: %.4f' % F1)
    if save_dir:
        nrrd_io.write(os.path.join(save_dir, 'segs.nrrd'), np.uint8(segs))
        np.savetxt(os.path.join(save_dir, 'F1_socre.txt'), [F1])
    return segs.astype(np.float64), F1


def DCRF_postprocess_2D(post_map, img_slice, sess=None):
    """PW_analyze_results.py:539-591: the dense CRF on one 2-D class-1 posterior map -> the [H, W] integer MAP labels.  Zeros
    of the caller's `post_map` become 1e-10, as the reference's in-place guard (:549) leaves them.  The model is the
    reference's (2 labels, smoothness sdims (1, 1) compat 20, appearance sdims (5, 5) schan 1 compat 30, NORMALIZE_SYMMETRIC,
    5 iterations, its unary [1 - nl, nl] as it stands); alq_dcrf2d evaluates it with exact Gaussian filters on the cut-off
    windows instead of pydensecrf's permutohedral lattice (dcrf.py).  `sess` (not a reference argument): the device session,
    default device.default_session()."""
    from . import device
    sess = sess or device.default_session()
    img_slice = np.asarray(img_slice)
    if img_slice.ndim != 2 or tuple(np.shape(post_map)) != img_slice.shape:
        raise ValueError('post_map %r and img_slice %r must be one 2-D shape' % (np.shape(post_map), img_slice.shape))
    labels = sess.dcrf2d(post_map, img_slice, img_slice.shape)
    return labels.cpu().numpy().reshape(img_slice.shape).astype(np.int64)


def full_model_pred_DCRF(expr, model, sess, img_path, mask_path, slice_inds, save_dir=None):
    """PW_analyze_results.py:449-536: the model's posteriors of every voxel of the slices `slice_inds`, post-processed slice by
    slice with the dense CRF, their F1 against the mask over those slices and, with `save_dir`, `dcrf_segs.nrrd` (uint8, as
    `segs.nrrd` is here) and `F1_score_dcrf.txt`.  Returns (DCRF_preds [x, y, z] float64, zero outside the slices, F1).

    The reference's call `full_slice_eval(model, img_path, [ind], 'axial', ...)` (:481-490) cannot run as written; the intent
    is restated exactly as full_model_eval does: expr.pars['patch_shape'], ['ntb'], ['stats'], all the modalities of
    `img_path` (one path / padded array, or a list of them).  The CRF's image is the first modality (the reference reads a
    single `img_path`).  Everything between the upload and the result stays on the device: posteriors_device fills one
    [S, H, W] tensor, the image slices are taken from the resident volume, ONE alq_dcrf2d call labels all slices, the labels
    are scattered into a uint8 volume and counted against the resident mask by alq_eval_counts; one volume of bytes and 48
    bytes of counts come back.  F1 is full_model_eval's: F1_scores' expression on those counts, 0 where its divisions
    would raise."""
    torch = sess.torch
    if save_dir:
        if not os.path.exists(save_dir):
            os.mkdir(save_dir)
    mask = mask_path if isinstance(mask_path, np.ndarray) else nrrd_io.read(mask_path)[0]
    img_paths = [img_path] if isinstance(img_path, (str, np.ndarray)) else list(img_path)
    patch_shape = expr.pars['patch_shape']
    vols, img_shape = _padded_volumes(img_paths, patch_shape)
    if tuple(mask.shape) != img_shape:
        raise ValueError('mask %r and image %r differ in shape' % (tuple(mask.shape), img_shape))
    slice_inds = [int(v) for v in slice_inds]
    H, W = img_shape[:2]
    S = len(slice_inds)
    seg = sess.to_device(np.zeros(img_shape, dtype=np.uint8), torch.uint8)
    F1 = 0
    if S:
        dv = patch_utils.DeviceVolumes(sess, vols)
        lab = _device_labels(sess, mask)
        post = sess.empty((S, H, W), torch.float32)
        inds = []
        for k, ind in enumerate(slice_inds):
            _, inds_3D = _slice_inds_3D(img_shape, ind)
            PW_NN.posteriors_device(model, sess, vols, inds_3D, patch_shape, expr.pars['ntb'], expr.pars['stats'], _vols=dv,
                                    out=post[k].reshape(-1))
            inds.append(inds_3D)
        rads = patch_utils.patch_radii(patch_shape)
        z = sess.to_device(np.asarray(slice_inds, dtype=np.int64) + rads[2], torch.int64)
        img = dv.tensors[0][rads[0]:rads[0] + H, rads[1]:rads[1] + W].index_select(2, z).permute(2, 0, 1).to(torch.float32).contiguous()
        labels = sess.dcrf2d(post, img, (S, H, W))
        seg[:, :, sess.to_device(np.asarray(slice_inds, dtype=np.int64), torch.int64)] = labels.permute(1, 2, 0)
        d_inds = sess.to_device(np.concatenate(inds), torch.int64)
        counts = sess.to_device(np.zeros(6, dtype=np.int64), torch.int64)
        sess.eval_counts(seg.reshape(-1)[d_inds].to(torch.int64), d_inds, lab.reshape(-1), counts, None)
        F1 = _f1_from_counts(counts)
    segs = seg.cpu().numpy().reshape(img_shape)
    if save_dir:
        nrrd_io.write(os.path.join(save_dir, 'dcrf_segs.nrrd'), np.uint8(segs))
        np.savetxt(os.path.join(save_dir, 'F1_score_dcrf.txt'), [F1])
    return segs.astype(np.float64), F1


def _f1_from_counts(counts):
    """F1_scores' expression on the six device totals of alq_eval_counts (one copy of 48 bytes); 0 without a true positive."""
    P, N, TP, FP, TN, FN = [float(v) for v in counts.cpu().numpy()]
    F1 = 0
    if TP > 0:                                                  # (then TP + FP > 0 and P > 0)
        Pr = TP / (TP + FP)
        Rc = TP / P
        F1 = 2 * Pr * Rc / (Pr + Rc)
    return F1


def eval_MultimgAL(expr, method_name, img_paths, start_ind=0, save_dir=[], sess=None):
    """PW_analyze_results.py:802-863: the learning curve of a method - for every iteration's `curr_weights_<i+1>` (through
    LoopState.weights_path: .h5 or the .npz twin) and every test subject j, scores[j, i] = expr.test_eval(model, sess)[0]
    with expr.test_paths = img_paths[j:j+1] and expr.test_stats = the mean / std of every modality over the non-NaN mask
    voxels (:850-857).  `<method>/test_scores.txt` is rewritten (np.savetxt, rank 0 only) after every entry; `start_ind` > 0
    resumes from that file.  Returns the score matrix (the reference returns nothing).  `save_dir` is unused there as here;
    `sess` (not a reference argument): the device session, default device.default_session()."""
    from . import PW_AL, device, pool_shard
    rank, _ = pool_shard.world()
    sess = sess or device.default_session()
    m = len(expr.train_paths[0]) - 1
    model = expr._create_model(sess)
    model.add_assign_ops()
    method_path = os.path.join(expr.root_dir, method_name)
    state = PW_AL.LoopState(method_path)
    qnum = len(get_queries(expr, method_name))
    imgnum = len(img_paths)
    save_dir = os.path.join(method_path, 'test_scores.txt')
    if start_ind > 0:
        scores = np.loadtxt(save_dir, ndmin=2).reshape(imgnum, -1)     # (one subject: savetxt dropped the dimension)
        if scores.shape[1] < qnum:                                     # iterations added since the file was written
            scores = np.concatenate([scores, np.zeros((imgnum, qnum - scores.shape[1]))], axis=1)
    else:
        scores = np.zeros((imgnum, qnum))
    pool_shard.barrier()                                               # every rank has read the file before rank 0 rewrites it
    for i in range(start_ind, qnum):
        weights_path = state.weights_path(i + 1)
        print('Loading weights %s' % weights_path)
        model.perform_assign_ops(weights_path, sess)
        for j in range(imgnum):
            expr.test_paths = img_paths[j:j + 1]
            stats_arr = np.zeros((1, 2 * m))
            mask = PW_AL._volume(expr.test_paths[0][-1])
            for t in range(m):
                img = PW_AL._volume(expr.test_paths[0][t])
                stats_arr[0, 2 * t:2 * (t + 1)] = np.array([np.mean(img[~np.isnan(mask)]), np.std(img[~np.isnan(mask)])])
            expr.test_stats = stats_arr
            scores[j, i], test_preds = expr.test_eval(model, sess)
            if rank == 0:
                np.savetxt(save_dir, scores)
            print(j, end=',')
        print()
    pool_shard.barrier()
    if hasattr(model, 'close'):
        model.close()                                                  # the model was created here: its device memory goes with it
    return scores
