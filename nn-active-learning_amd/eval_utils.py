"""Evaluation of fully-convolutional models (reference module: eval_utils.py) - whole-volume segmentation slice by slice, F1
scores and the validation-metric bookkeeping - written against `model.posteriors` of shape [N, *spatial, c].

`model` is a dense NN_extended.CNN / device.DeviceModel (1x1 conv head) and `sess` its DeviceSession; any object pair with the
same protocol works (`model.in_shape`, the handles `x`, `keep_prob`, `posteriors`, `loss`, `y_`, and `sess.run`), which is
what the host tests use.  On a device model the slices' outputs stay on the device and the assembled volume is copied back
once; F1 scores come from a confusion matrix (no scikit-learn import)."""
import os

import numpy as np

SLICE_BATCH = 4       # slices per sess.run of full_slice_segment
MC_PASSES = 10        # dropout passes of the 'MC-posterior' op


def gen_batch_inds(data_size, batch_size):
    """A random partition of range(data_size) into index lists of `batch_size`, the remainder as a last, shorter list (drawn
    from the global np.random stream, one permutation per call)."""
    perm = np.random.permutation(int(data_size)).tolist()
    full = int(data_size) // int(batch_size)
    batches = [perm[i * batch_size:(i + 1) * batch_size] for i in range(full)]
    if full * batch_size < data_size:
        batches.append(perm[full * batch_size:])
    return batches


def _on_device(model):
    return bool(getattr(model, 'dense', False)) and hasattr(model, 'forward_maps_device')


def _load_volumes(img_paths_or_mats, data_reader):
    """-> list of m arrays (h, w, z): one per input channel."""
    items = img_paths_or_mats if isinstance(img_paths_or_mats, list) else [img_paths_or_mats]
    return [it if isinstance(it, np.ndarray) else data_reader(it) for it in items]


def full_slice_segment(model, sess, img_paths_or_mats, data_reader, op='prediction', mask=None):
    """Runs `op` over every z slice of a volume, SLICE_BATCH slices per run (a random partition, each batch in ascending slice
    order), and assembles the result in the volume's own layout.

    img_paths_or_mats: one (h, w, z) array or path, or a list of m of them (the m input channels, stacked last).
    op: 'prediction' -> (h, w, z) argmax of the posteriors; 'posterior' -> (c, h, w, z); 'MC-posterior' -> (c, h, w, z), the
    running mean of MC_PASSES passes at keep_prob = 1 - model.dropout_rate; 'loss' -> the slice-weighted running mean of
    model.loss (needs `mask`: the (h, w, z) label volume, fed one-hot under model.y_; a model whose loss takes no labels may
    leave it out).  A model with AU_4U true (eval_utils.py:147-198): 'AU_vals' -> (h, w, z), the log-variance map; 'output' ->
    (c + 1, h, w, z), the head's raw channels; 'sigma' -> (c, h, w, z), the raw log-variance channel broadcast over c as the
    reference's assignment does; 'MC-sigma' -> the same of its running mean over MC_PASSES dropout passes.  These four run
    through sess.run and are assembled on the host; any other model: NotImplementedError."""
    au_op = op in ('output', 'AU_vals', 'sigma', 'MC-sigma')
    if au_op and not getattr(model, 'AU_4U', False):
        raise NotImplementedError('op %r needs a model with AU_4U (an aleatoric-uncertainty head)' % (op,))
    if not au_op and op not in ('prediction', 'posterior', 'MC-posterior', 'loss'):
        raise ValueError('unknown op %r' % (op,))
    imgs = _load_volumes(img_paths_or_mats, data_reader)
    m = len(imgs)
    h, w, z = imgs[0].shape
    hx, wx = int(model.in_shape[0]), int(model.in_shape[1])
    assert h == hx and w == wx, 'Shape of data and model.x should match.'
    c = int(getattr(model, 'class_num', getattr(model, 'nclass', 0)))
    dev = _on_device(model) and op != 'loss' and not au_op
    if dev:
        torch = sess.torch
        vols = sess.to_device(np.stack([np.asarray(v, dtype=np.float32) for v in imgs], axis=-1), torch.float32)      # (h, w, z, m)
        out = torch.zeros((h, w, z), dtype=torch.int64, device=vols.device) if op == 'prediction' else \
            torch.zeros((c, h, w, z), dtype=torch.float32, device=vols.device)
    elif op in ('prediction', 'AU_vals'):
        out = np.zeros((h, w, z))
    elif op == 'output':
        out = np.zeros((c + 1, h, w, z))
    elif op == 'loss':
        out, seen = 0., 0
    else:
        out = np.zeros((c, h, w, z))

    def posteriors(batch_X, keep_prob):
        """[b, h, w, c]: a device tensor on the device path, else what sess.run returns."""
        if dev:
            return model.forward_maps_device(batch_X, int(batch_X.shape[0]), keep_prob)[0]
        return np.asarray(sess.run(model.posteriors, feed_dict={model.x: batch_X, model.keep_prob: keep_prob}))

    for batch in gen_batch_inds(z, SLICE_BATCH):
        inds = np.sort(np.asarray(batch, dtype=np.int64))
        if dev:
            di = torch.as_tensor(inds, device=vols.device)
            batch_X = vols[:, :, di, :].permute(2, 0, 1, 3).contiguous()
        else:
            batch_X = np.zeros((len(inds), h, w, m))
            for j in range(m):
                batch_X[:, :, :, j] = np.moveaxis(np.asarray(imgs[j])[:, :, inds], -1, 0)
        if op == 'loss':
            feed = {model.x: batch_X, model.keep_prob: 1.}
            if mask is not None:
                lab = np.moveaxis(np.asarray(mask)[:, :, inds], -1, 0).astype(np.int64)
                feed[model.y_] = (lab[..., None] == np.arange(c)).astype(np.float32)
            val = float(sess.run(model.loss, feed_dict=feed))
            out = (len(inds) * val + seen * out) / (seen + len(inds))
            seen += len(inds)
            continue
        if au_op:
            kp = 1. - float(model.dropout_rate) if op == 'MC-sigma' else 1.
            fetch = model.AU_vals if op == 'AU_vals' else model.output
            run = lambda: np.asarray(sess.run(fetch, feed_dict={model.x: batch_X, model.keep_prob: kp}))
            if op == 'AU_vals':
                out[:, :, inds] = np.transpose(run(), (1, 2, 0))
                continue
            P = run()
            if op != 'output':          # the one raw channel behind the classes, [b, h, w, 1]
                P = P[..., c:]
                for i in range(1, MC_PASSES if op == 'MC-sigma' else 1):
                    P = (i * P + run()[..., c:]) / (i + 1)
            out[:, :, :, inds] = np.transpose(P, (3, 1, 2, 0))          # ('sigma': broadcast over the c planes)
            continue
        if op == 'MC-posterior':
            kp = 1. - float(model.dropout_rate)
            P = posteriors(batch_X, kp)
            for i in range(1, MC_PASSES):
                P = (i * P + posteriors(batch_X, kp)) / (i + 1)
        else:
            P = posteriors(batch_X, 1.)
        if op == 'prediction':
            if dev:
                out[:, :, di] = P.argmax(dim=-1).permute(1, 2, 0)
            else:
                out[:, :, inds] = np.moveaxis(np.argmax(P, axis=-1), 0, -1)
        elif dev:
            out[:, :, :, di] = P.permute(3, 1, 2, 0)
        else:
            out[:, :, :, inds] = np.transpose(P, (3, 1, 2, 0))
    if dev:
        return out.cpu().numpy().astype(np.float64)        # one copy; np.zeros volumes of the host path are float64 too
    return out


def confusion_matrix(preds, labels, C):
    """counts[t, p] over the flattened label maps; values outside [0, C) are left out."""
    p = np.ravel(np.asarray(preds)).astype(np.int64)
    t = np.ravel(np.asarray(labels)).astype(np.int64)
    ok = (p >= 0) & (p < C) & (t >= 0) & (t < C)
    return np.bincount(t[ok] * C + p[ok], minlength=C * C).reshape(C, C)


MAX_DEVICE_CLASSES = 16       # alq_confusion_counts: 1 <= C <= 16


def confusion_counts_host(pred, labels, C, inner=None, groups=1, first=0, fill=-1, want_skipped=False):
    """alq_confusion_counts in NumPy: np.int64 [groups, C, C], counts[g][t][p] over the flattened id arrays with
    g = ((first + i) // inner) % groups (inner None: one run, inner = n).  A label outside [0, C) reads as `fill` when
    0 <= fill < C; an element whose label (after that) or prediction lies outside [0, C) is skipped.  want_skipped:
    (counts, number of skipped elements)."""
    p = np.ravel(np.asarray(pred)).astype(np.int64)
    t = np.ravel(np.asarray(labels)).astype(np.int64)
    C, groups = int(C), int(groups)
    n = p.size
    inner = max(n, 1) if inner is None else int(inner)
    g = ((int(first) + np.arange(n, dtype=np.int64)) // inner) % groups
    if 0 <= int(fill) < C:
        t = np.where((t < 0) | (t >= C), int(fill), t)
    ok = (p >= 0) & (p < C) & (t >= 0) & (t < C)
    counts = np.bincount((g[ok] * C + t[ok]) * C + p[ok], minlength=groups * C * C).reshape(groups, C, C).astype(np.int64)
    return (counts, int(n - np.count_nonzero(ok))) if want_skipped else counts


def F1_from_confusion(M, C=None):
    """The F1 arithmetic of binary_F1_score and multi_F1_score on a confusion matrix M[t, p] (any square integer matrix that
    spans the values present) -> (binary, scores, average):
      binary   2 TP / (P + TPFP) with TP = sum t p M[t, p], P = sum t M[t, p], TPFP = sum p M[t, p] - np.sum(preds * labels),
               np.sum(labels) and np.sum(preds) of the maps M counts, for any integer values; 0. when P + TPFP is 0;
      scores   per-class F1 of the classes 1 .. C-1 (C None: the matrix' size), 0 for a class with no true and no predicted voxel;
      average  their support-weighted mean, 0 without support."""
    M = np.asarray(M, dtype=np.int64)
    span = M.shape[0]
    vals = np.arange(span, dtype=np.int64)
    TP = np.sum(np.outer(vals, vals) * M)
    den = np.sum(vals * M.sum(axis=1)) + np.sum(vals * M.sum(axis=0))
    binary = 2 * TP / den if den != 0 else 0.
    C = span if C is None else int(C)
    scores = np.zeros(max(C - 1, 0))
    support = np.zeros(max(C - 1, 0))
    for j in range(1, min(C, span)):
        d = M[j, :].sum() + M[:, j].sum()
        scores[j - 1] = 2. * M[j, j] / d if d else 0.
        support[j - 1] = M[j, :].sum()
    av = float(np.sum(scores * support) / support.sum()) if support.sum() else 0.
    return binary, scores, av


def _countable(preds, labels):
    """True when both maps hold integers in [0, 2^16) and np.sum(preds * labels) cannot wrap in their common dtype: their
    products and sums can then be read off a confusion matrix.  (A product of two uint8 maps with values above 15 wraps in the
    reference's np.sum(preds * labels); such maps keep that statement.)"""
    for a in (preds, labels):
        if a.size == 0 or a.dtype.kind == 'b':
            continue
        if a.dtype.kind not in 'iu' and (a.dtype.kind != 'f' or not np.all(a == np.floor(a))):
            return False
        if a.min() < 0 or a.max() >= 65536:
            return False
    dt = np.result_type(preds, labels)
    if dt.kind in 'iu' and preds.size and labels.size and int(preds.max()) * int(labels.max()) > np.iinfo(dt).max:
        return False
    return True


def binary_F1_score(preds, labels):
    """2 TP / (P + TPFP) of two 0/1 maps; 0 when neither holds a positive.  TP = np.sum(preds * labels), P = np.sum(labels),
    TPFP = np.sum(preds), as the reference states it: integer maps are counted into a confusion matrix and scored by
    F1_from_confusion (the same doubles), anything else takes the three sums themselves."""
    preds, labels = np.asarray(preds), np.asarray(labels)
    if preds.shape == labels.shape and _countable(preds, labels):
        span = 1 + int(max(preds.max() if preds.size else 0, labels.max() if labels.size else 0))
        if span * span <= 4096:
            return F1_from_confusion(confusion_matrix(preds, labels, span))[0]
    TP = np.sum(preds * labels)
    den = np.sum(labels) + np.sum(preds)
    return 2 * TP / den if den != 0 else 0.


def multi_F1_score(preds, labels, C=None):
    """(per-class F1 of the classes 1 .. C-1, their support-weighted mean): class 0, the background, is no class of its own in
    the average.  A class with no true and no predicted voxel scores 0; no support at all gives an average of 0.  C defaults
    to the number of distinct labels."""
    if C is None:
        C = len(np.unique(labels))
    C = int(C)
    p = np.ravel(np.asarray(preds)).astype(np.int64)
    t = np.ravel(np.asarray(labels)).astype(np.int64)
    # every voxel counts, whatever its other value is: the matrix spans all values present, the scores read classes 1 .. C-1
    span = max(C, int(p.max()) + 1 if p.size else 0, int(t.max()) + 1 if t.size else 0)
    _, scores, av = F1_from_confusion(confusion_matrix(p, t, span), C)
    return scores, av


def _confusion_pass(model, sess, dat_gen, iters, want_loss, want_counts):
    """`iters` batches through a dense device model: (np.int64 [C, C] confusion matrix [true, predicted] or None, the batch-size-
    weighted mean of model.loss or None).  Predictions come from forward_maps_device(want_pred=True) and never leave the
    device; labels are DeviceLabels.labels in place, or a host one-hot reduced to int32 ids once and uploaded; an unlabelled
    voxel (-1, or an all-zero one-hot row) is class 0, np.argmax's reading of it.  One confusion_counts call per batch into one
    resident matrix, one download of 8 C^2 bytes at the end."""
    torch = sess.torch
    C = int(getattr(model, 'class_num', getattr(model, 'nclass', 0)))
    counts = torch.zeros((1, C, C), dtype=torch.int64, device=sess.device) if want_counts else None
    av_loss, vol = (0. if want_loss else None), 0
    for _ in range(iters):
        batch_X, batch_mask = dat_gen()
        b = batch_X.shape[0]
        if want_loss:
            val = float(sess.run(model.loss, feed_dict={model.x: batch_X, model.y_: batch_mask, model.keep_prob: 1.}))
            av_loss = (vol * av_loss + val * b) / (vol + b)
        if want_counts:
            t, n = model._as_device_batch(batch_X)
            pred = model.forward_maps_device(t, n, 1., want_pred=True)[1]
            if model._is_device_labels(batch_mask):
                lab = batch_mask.labels.to(device=sess.device, dtype=torch.int32).contiguous()
            else:
                lab = sess.to_device(np.argmax(np.asarray(batch_mask), axis=-1).astype(np.int32), torch.int32)
            sess.confusion_counts(pred.contiguous(), lab, C, fill=0, counts=counts)
        vol += b
    return (counts.cpu().numpy().reshape(C, C) if want_counts else None), av_loss


def eval_confusion(model, sess, dat_gen, iters=50):
    """The confusion matrix of `iters` batches of `dat_gen()` -> (batch_X, batch_mask): np.int64 [C, C], indexed
    [true, predicted].  A dense device model counts on the device (_confusion_pass); any other model runs model.posteriors
    through sess.run and counts with NumPy - the same matrix."""
    C = int(getattr(model, 'class_num', getattr(model, 'nclass', 0)))
    if _on_device(model):
        return _confusion_pass(model, sess, dat_gen, iters, False, True)[0]
    M = np.zeros((C, C), dtype=np.int64)
    for _ in range(iters):
        batch_X, batch_mask = dat_gen()
        feed = {model.x: batch_X, model.y_: batch_mask, model.keep_prob: 1.}
        preds = np.argmax(np.asarray(sess.run(model.posteriors, feed_dict=feed)), axis=-1)
        M += confusion_matrix(preds, np.argmax(np.asarray(batch_mask), axis=-1), C)
    return M


def eval_metrics(model, sess, dat_gen, iters=50, update=True, alt_attr=None):
    """`iters` batches of `dat_gen()` -> (batch_X, one-hot batch_mask [b, *spatial, c]) through the model; the metrics named
    by the keys of `model.valid_metrics` (or of the attribute `alt_attr`): 'acc' / 'av_acc' (voxel accuracy), 'F1' (binary, or
    the weighted multi-class score) and 'av_loss' (batch-size-weighted mean of model.loss).  update=True appends one value
    per metric to its list; otherwise the running results are returned.  A dense device model counts on the device
    (eval_confusion's matrix: no posterior map and no label crosses to the host); both paths score the matrix with
    F1_from_confusion."""
    if alt_attr is not None:
        assert hasattr(model, alt_attr), 'The alternative attribute does not exist.'
        valid_metrics = getattr(model, alt_attr)
    else:
        valid_metrics = model.valid_metrics
    names = list(valid_metrics.keys())
    C = int(getattr(model, 'class_num', getattr(model, 'nclass', 0)))
    want_post = any(k in names for k in ('acc', 'av_acc', 'F1'))
    want_loss = 'av_loss' in names
    results = {}
    if want_loss:
        results['av_loss'] = 0.
    if _on_device(model) and hasattr(sess, 'confusion_counts') and 1 <= C <= MAX_DEVICE_CLASSES:
        M, av_loss = _confusion_pass(model, sess, dat_gen, iters, want_loss, want_post)
        if want_loss:
            results['av_loss'] = av_loss
    else:
        M = None
        all_preds, all_masks = [], []
        vol = 0
        for _ in range(iters):
            batch_X, batch_mask = dat_gen()
            b = batch_X.shape[0]
            feed = {model.x: batch_X, model.y_: batch_mask, model.keep_prob: 1.}
            if want_loss:
                val = float(sess.run(model.loss, feed_dict=feed))
                results['av_loss'] = (vol * results['av_loss'] + val * b) / (vol + b)
            if want_post:
                all_preds.append(np.argmax(np.asarray(sess.run(model.posteriors, feed_dict=feed)), axis=-1))
                all_masks.append(np.argmax(batch_mask, axis=-1))
            vol += b
        if want_post:
            preds, masks = np.concatenate(all_preds, axis=0), np.concatenate(all_masks, axis=0)
            # the matrix spans every value present, as multi_F1_score's does; the scores read classes 1 .. C-1
            M = confusion_matrix(preds, masks, max(C, int(preds.max()) + 1 if preds.size else 0, int(masks.max()) + 1 if masks.size else 0))
    if want_post:
        total = int(M.sum())
        results['accs'] = float(np.trace(M)) / total if total else 0.
        results['F1s'] = F1_from_confusion(M, C)[0] if C == 2 else F1_from_confusion(M, C)[2]
    if not update:
        return results
    for name in names:
        if name in ('acc', 'av_acc'):
            valid_metrics[name] += [results['accs']]
        elif name == 'F1':
            valid_metrics[name] += [results['F1s']]
        elif 'loss' in name and name in results:
            valid_metrics[name] += [results[name]]


def get_full_segs(models_dict, sess, dat, post_process=False, save_path=None, dat_writer=None):
    """The segmentation of every subject of `dat` (attributes img_addrs {modality: [paths]}, mods, mask_addrs, mask_reader,
    reader): the model is looked up in `models_dict` under str((h, w)) of the subject's mask; post_process=True keeps the
    largest connected component and fills its holes (post_processing.py, on the device).  save_path: an existing directory
    the volumes are written to as seg_<i>.nrrd through `dat_writer(path, volume)` (default: nrrd_io.write)."""
    from .post_processing import connected_component_analysis_3d, fill_holes
    n = len(dat.img_addrs[dat.mods[0]])
    segs = []
    for i in range(n):
        shape = tuple(dat.mask_reader(dat.mask_addrs[i]).shape[:2])
        model = models_dict['{}'.format(shape)]
        seg = full_slice_segment(model, sess, [dat.img_addrs[mod][i] for mod in dat.mods], dat.reader)
        if post_process:
            seg = fill_holes(connected_component_analysis_3d(seg, sess=sess), sess=sess)
        segs.append(seg)
    if save_path is not None:
        if not os.path.exists(save_path):
            print('The specified path for saving data does not exist.')
            return segs
        if dat_writer is None:
            from . import nrrd_io
            dat_writer = nrrd_io.write
        for i, seg in enumerate(segs):
            dat_writer(os.path.join(save_path, 'seg_{}.nrrd'.format(i)), seg)
    return segs


def _tile_geometry(model, stride):
    """(tile, stride) of a dense model, each (Z, H, W): a 3-D model of in_shape (D, H, W, m) tiles the volume by (D, H, W) blocks, a
    2-D one of (h, w, m) by (1, h, w) - every axial slice, stride 1 along z.  stride None: half a tile per axis (at least 1); an
    int: that many voxels on every in-plane axis; a sequence: one value per spatial axis of the model."""
    from . import tiled
    spatial = tuple(int(v) for v in model.in_shape[:-1])
    if len(spatial) not in (2, 3):
        raise NotImplementedError('full_volume_segment: a model of input shape %r' % (tuple(model.in_shape),))
    if stride is None:
        st = tiled.default_stride(spatial)
    elif np.ndim(stride) == 0:
        st = (int(stride),) * len(spatial)
    else:
        st = tuple(int(v) for v in stride)
        if len(st) != len(spatial):
            raise ValueError('stride %r for a model with %d spatial axes' % (stride, len(spatial)))
    if len(spatial) == 2:
        return (1,) + spatial, (1,) + st
    return spatial, st


def full_volume_segment(model, sess, img_paths_or_mats, data_reader=None, op='prediction', stride=None, window='gaussian', fill=0.,
                        keep_on_device=False):
    """Runs a dense device model over a whole volume of ANY size by overlapping tiles of the model's input shape and blends the
    tiles' posteriors on the device (tiled.py states every operation; csrc/tile.hip).

    img_paths_or_mats: one (h, w, z) array or path, a list of m of them, or a datasets.utils.ResidentSubject (read in place).
    op: 'prediction' -> (h, w, z), the first maximum of the blended posteriors; 'posterior' -> (c, h, w, z); 'MC-posterior' ->
    (c, h, w, z) of the running mean of MC_PASSES dropout passes per tile at keep_prob = 1 - model.dropout_rate, the masks keyed by
    (pass seed, tile index) - the MC_PASSES seeds are drawn from np.random once, so the result does not depend on model.max_batch.
    stride: see _tile_geometry.  window: 'uniform', 'triangle' or 'gaussian' (tiled.window).  fill: the value of input voxels
    outside the volume (only where the volume is smaller than the tile).  Float64 NumPy as full_slice_segment returns;
    keep_on_device=True: the uint8 [h, w, z] / float32 [c, h, w, z] device tensors.  A model with AU_4U is served on its c clean
    channels; an fc-head model raises NotImplementedError."""
    from . import tiled
    from .datasets.utils import ResidentSubject
    if op not in ('prediction', 'posterior', 'MC-posterior'):
        raise ValueError('unknown op %r' % (op,))
    if not _on_device(model):
        raise NotImplementedError('full_volume_segment needs a fully-convolutional device model (1x1 conv head)')
    tile, st = _tile_geometry(model, stride)
    if tuple(int(v) for v in model.out_map_shape) != tuple(int(v) for v in model.in_shape[:-1]):
        raise NotImplementedError('full_volume_segment: the output map %r is not the input grid %r' % (model.out_map_shape, model.in_shape[:-1]))
    torch = sess.torch
    if isinstance(img_paths_or_mats, ResidentSubject):
        subject = img_paths_or_mats
    else:
        subject = ResidentSubject.pack(sess, _load_volumes(img_paths_or_mats, data_reader))
    h, w, z = subject.shape
    if subject.m != int(model.in_shape[-1]):
        raise ValueError('the subject has %d channels, the model takes %d' % (subject.m, int(model.in_shape[-1])))
    c = int(model.class_num)
    lat = sess.tile_lattice((z, h, w), tile, st)
    ntiles = sess.tile_count(lat)
    windows = tuple(sess.to_device(tiled.window(window, t), torch.float32) for t in tile)
    acc = torch.zeros((c + 1, z, h, w), dtype=torch.float32, device=sess.device)
    mc = op == 'MC-posterior'
    kp = 1. - float(model.dropout_rate) if mc else 1.
    seeds = [int(np.random.randint(0, 2 ** 31 - 1)) for _ in range(MC_PASSES)] if mc else [None]
    nb = int(model.max_batch)
    X = sess.empty((min(nb, ntiles),) + tuple(tile) + (subject.m,), torch.float32)
    for first in range(0, ntiles, nb):
        n = min(nb, ntiles - first)
        Xn = sess.tile_gather(subject.vol, lat, first, n, fill, out=X[:n])
        P = None
        for i, seed in enumerate(seeds):
            # [c, n V]: the class-major planes the library wrote, before forward_maps_device's movedim view
            Pi = model.forward_maps_device(Xn, n, kp, seed=seed, first_sample=first)[0].movedim(-1, 0).reshape(c, -1)
            P = Pi if P is None else (i * P + Pi) / (i + 1)
        sess.tile_blend(P.contiguous(), lat, first, n, windows, acc)
    want_post = op != 'prediction'
    post, label = sess.tile_finalize(acc, hwz=True, want_post=want_post, want_label=not want_post)
    out = post if want_post else label
    if keep_on_device:
        return out
    return out.cpu().numpy().astype(np.float64)


def get_full_segs_tiled(model, sess, dat, stride=None, window='gaussian', post_process=False, save_path=None, dat_writer=None):
    """get_full_segs with ONE model for every subject size (full_volume_segment instead of a dictionary of models per size).
    post_process=True keeps the largest connected component and fills its holes on the label volume where it lies (the uint8
    [h, w, z] device tensor full_volume_segment leaves; post_processing.py); the segmentations are np.uint32 then, as
    post_processing returns them."""
    from .post_processing import connected_component_analysis_3d, fill_holes
    n = len(dat.img_addrs[dat.mods[0]])
    segs = []
    for i in range(n):
        seg = full_volume_segment(model, sess, [dat.img_addrs[mod][i] for mod in dat.mods], dat.reader, stride=stride, window=window,
                                  keep_on_device=True)
        if post_process:
            shape = tuple(int(v) for v in seg.shape)
            seg = fill_holes(connected_component_analysis_3d(seg, sess=sess, shape=shape), sess=sess, shape=shape)
            segs.append(seg.cpu().numpy().astype(np.uint32))
        else:
            segs.append(seg.cpu().numpy().astype(np.float64))
    _save_segs(segs, save_path, dat_writer)
    return segs


def _save_segs(segs, save_path, dat_writer):
    """seg_<i>.nrrd under the existing directory `save_path` through `dat_writer(path, volume)` (default: nrrd_io.write)."""
    if save_path is None:
        return
    if not os.path.exists(save_path):
        print('The specified path for saving data does not exist.')
        return
    if dat_writer is None:
        from . import nrrd_io
        dat_writer = nrrd_io.write
    for i, seg in enumerate(segs):
        dat_writer(os.path.join(save_path, 'seg_{}.nrrd'.format(i)), seg)


# ---- whole-volume scores by axial partitions (eval_utils.py:240-363) --------------------------------------------------------
def _load_list(paths_or_mats, reader):
    if isinstance(paths_or_mats[0], str):
        return [reader(path) for path in paths_or_mats]
    return paths_or_mats


def _readers(kwargs):
    from . import nrrd_io
    kwargs.setdefault('dat_reader', lambda x: nrrd_io.read(x)[0])
    kwargs.setdefault('mask_reader', lambda x: nrrd_io.read(x)[0])
    return kwargs['dat_reader'], kwargs['mask_reader'], kwargs.get('sess')


class _SliceScores(object):
    """binary_F1_score of any range of axial slices of one (seg, mask) pair, and the per-slice count of a mask label, from the
    per-slice confusion counts [Z, C, C] (counts[z][mask value][seg value], C = the largest value + 1): with a session one
    alq_confusion_counts launch over the two uint8 volumes (inner = 1, groups = Z: z is the fastest axis), else
    confusion_counts_host; values above 15 count with NumPy too.  Maps that hold anything but non-negative integers keep the
    reference's own sums on the slices."""

    def __init__(self, seg, mask, sess):
        self.seg, self.mask = np.asarray(seg), np.asarray(mask)
        self.counts = None
        if self.seg.shape != self.mask.shape or self.seg.ndim != 3 or not self.seg.size or not _countable(self.seg, self.mask):
            return
        Z = self.seg.shape[2]
        C = 1 + int(max(self.seg.max(), self.mask.max()))
        if C > 256:
            return
        if sess is not None and C <= MAX_DEVICE_CLASSES:
            torch = sess.torch
            d_seg = sess.to_device(self.seg.astype(np.uint8), torch.uint8)
            d_mask = sess.to_device(self.mask.astype(np.uint8), torch.uint8)
            self.counts = sess.confusion_counts(d_seg, d_mask, C, inner=1, groups=Z).cpu().numpy()
        else:
            self.counts = confusion_counts_host(self.seg, self.mask, C, inner=1, groups=Z)

    def score(self, lo=None, hi=None):
        """binary_F1_score(seg[:, :, lo:hi], mask[:, :, lo:hi])"""
        if self.counts is None:
            return binary_F1_score(self.seg[:, :, lo:hi], self.mask[:, :, lo:hi])
        return F1_from_confusion(self.counts[lo:hi].sum(axis=0))[0]

    def label_num(self, label):
        """np.sum(mask == label, axis=(0, 1))"""
        if self.counts is None:
            return np.sum(self.mask == label, axis=(0, 1))
        C = self.counts.shape[1]
        if label != int(label) or not 0 <= int(label) < C:
            return np.zeros(self.counts.shape[0], dtype=np.int64)
        return self.counts[:, int(label), :].sum(axis=1)


def eval_full_segs_explicit_partitions(seg_paths_or_mats, mask_paths_or_mats, slice_partitions, **kwargs):
    """(overall F1 [n], partition F1 [n, M]) of n whole-volume segmentations against their masks: binary_F1_score of each volume
    and of the M = (cut points + 1) ranges of axial slices that `slice_partitions` cuts it into - an int array [n, M - 1], or a
    list, which is np.repeat(np.array(list), n, axis=0) as in the reference (so the list is nested: [[c0, c1, ..]]).
    Keywords: dat_reader / mask_reader for paths (default nrrd_io.read) and sess - with a session the counting runs on the
    device (_SliceScores)."""
    dat_reader, mask_reader, sess = _readers(kwargs)
    segs = _load_list(seg_paths_or_mats, dat_reader)
    masks = _load_list(mask_paths_or_mats, mask_reader)
    if isinstance(slice_partitions, list):
        slice_partitions = np.repeat(np.array(slice_partitions), len(segs), axis=0)
    M = slice_partitions.shape[1] + 1
    part_Fscores = np.zeros((len(segs), M))
    overall_Fscores = np.zeros(len(segs))
    for i in range(len(segs)):
        sc = _SliceScores(segs[i], masks[i], sess)
        overall_Fscores[i] = sc.score()
        part_Fscores[i, 0] = sc.score(None, slice_partitions[i, 0])
        for j in range(slice_partitions.shape[1] - 1):
            part_Fscores[i, j + 1] = sc.score(slice_partitions[i, j], slice_partitions[i, j + 1])
        part_Fscores[i, -1] = sc.score(slice_partitions[i, -1], None)
    return overall_Fscores, part_Fscores


def eval_full_segs_label_percentage(seg_paths_or_mats, mask_paths_or_mats, label, percentage, **kwargs):
    """(overall F1 [n], partition F1 [n, 3]): the three-fold partition of the axial slices at the one gap of the set of slices
    whose share of `label` voxels lies below `percentage` (top, middle, bottom).  As in the reference: more than one gap
    prints its message and leaves the subject's row zero; no gap at all is its IndexError.  Keywords as above."""
    dat_reader, mask_reader, sess = _readers(kwargs)
    segs = _load_list(seg_paths_or_mats, dat_reader)
    masks = _load_list(mask_paths_or_mats, mask_reader)
    M = 3
    part_Fscores = np.zeros((len(segs), M))
    overall_Fscores = np.zeros(len(segs))
    for i in range(len(segs)):
        sc = _SliceScores(segs[i], masks[i], sess)
        overall_Fscores[i] = sc.score()
        label_num = sc.label_num(label)
        thr_slices = np.where(label_num / np.prod(np.asarray(masks[i]).shape[:2]) < percentage)[0]
        gap_loc = np.where((thr_slices[1:] - thr_slices[:-1]) > 1)[0]
        if len(gap_loc) > 1:
            print('There are more than one gap for slice-wise label volume' + ' of image {}'.format(i))
            continue
        edge_1 = thr_slices[gap_loc[0]]
        edge_2 = thr_slices[gap_loc[0] + 1]
        part_Fscores[i, 0] = sc.score(None, edge_1)
        part_Fscores[i, 1] = sc.score(edge_1, edge_2)
        part_Fscores[i, 2] = sc.score(edge_2, None)
    return overall_Fscores, part_Fscores


def eval_full_segs_surface_distances(seg_paths_or_mats, mask_paths_or_mats, spacings=None, labels=None, percentile=95., **kwargs):
    """Boundary metrics (surfdist.surface_distances: HD, HD95, ASSD, MHD, surface voxel counts, directed values) of n whole-volume
    segmentations against their masks: a dict of arrays [n], or [n, len(labels)] when `labels` lists the mask values to score
    one by one (None: foreground is != 0).  `spacings`: one (h, w, z) for all, or one per subject; None: ones for arrays, and for
    paths read with the default mask_reader the spacing of each mask file, nrrd_io.voxel_spacing(header).
    Keywords: dat_reader / mask_reader for paths (default nrrd_io.read) and sess - with a session each volume is uploaded
    once and every label is scored on the device (HD95 is the maximum of the directed percentiles, surfdist's module text)."""
    from . import nrrd_io, surfdist
    default_reader = 'mask_reader' not in kwargs
    dat_reader, mask_reader, sess = _readers(kwargs)
    segs = _load_list(seg_paths_or_mats, dat_reader)
    masks = _load_list(mask_paths_or_mats, mask_reader)
    n = len(segs)
    if spacings is None:
        spacings = [(1., 1., 1.)] * n
        if default_reader and n and isinstance(mask_paths_or_mats[0], str):
            spacings = []
            for path in mask_paths_or_mats:
                with open(path, 'rb') as f:
                    spacings.append(nrrd_io.voxel_spacing(nrrd_io.read_header(f)))
    elif np.ndim(spacings) == 1:
        spacings = [tuple(spacings)] * n
    labs = [None] if labels is None else list(labels)
    out = {}
    for i in range(n):
        seg, mask = np.asarray(segs[i]), np.asarray(masks[i])
        sp = tuple(spacings[i])[:seg.ndim]
        if sess is not None:
            # one upload per volume, every label reads it in place
            shape = seg.shape
            binary = labels is None
            seg = sess.to_device((seg != 0) if binary else seg, sess.torch.uint8)
            mask = sess.to_device((mask != 0) if binary else mask, sess.torch.uint8)
        for j, lab in enumerate(labs):
            res = surfdist.surface_distances(seg, mask, sp, lab, percentile, sess, shape if sess is not None else None)
            for k, v in res.items():
                if k not in out:
                    out[k] = np.zeros((n, len(labs)), dtype=np.int64 if k.startswith('n_') else np.float64)
                out[k][i, j] = v
    if labels is None:
        out = {k: v[:, 0] for k, v in out.items()}
    return out


def simple_eval_model(model, sess, dat_gen):
    """(accuracy, predictions) over the batches (Xb, Yb, _) of the iterable `dat_gen` (eval_utils.py:391-409): model.prediction
    at keep_prob 1 (no keep_prob in the feed when model.dropout_rate is None), the ground truth np.argmax(Yb, axis=0) - class
    scores along the first axis."""
    preds, grounds = [], []
    feed_dict = {} if model.dropout_rate is None else {model.keep_prob: 1.}
    for Xb, Yb, _ in dat_gen:
        feed_dict.update({model.x: Xb})
        preds += [sess.run(model.prediction, feed_dict=feed_dict)]
        grounds += [np.argmax(Yb, axis=0)]
    preds = np.concatenate(preds)
    grounds = np.concatenate(grounds)
    acc = np.sum(preds == grounds) / len(preds)
    return acc, preds


def models_dict_for_different_sizes(model_builder, dat):
    """{str((h, w)): model_builder([h, w], '<h>x<w>')} with one model per distinct in-plane image size of `dat` (read through
    dat.reader from dat.img_addrs[dat.mods[0]]): the dictionary get_full_segs looks its models up in.  The reference's
    np.unique(set(shapes))[0] is read as "the set of distinct shapes", here in sorted order; add_assign_ops() is called where the
    model has it."""
    shapes = []
    for i in range(len(dat.img_addrs[dat.mods[0]])):
        img = dat.reader(dat.img_addrs[dat.mods[0]][i])
        shapes += [tuple(int(v) for v in img.shape[:2])]
    models_dict = {}
    for shape in sorted(set(shapes)):
        key = str(shape)
        model_name = '{}x{}'.format(shape[0], shape[1])
        models_dict[key] = model_builder(list(shape), model_name)
        if hasattr(models_dict[key], 'add_assign_ops'):
            models_dict[key].add_assign_ops()
    return models_dict
