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


def binary_F1_score(preds, labels):
    """2 TP / (P + TPFP) of two 0/1 maps; 0 when neither holds a positive."""
    preds, labels = np.asarray(preds), np.asarray(labels)
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
    M = confusion_matrix(p, t, span)
    scores = np.zeros(max(C - 1, 0))
    support = np.zeros(max(C - 1, 0))
    for j in range(1, C):
        den = M[j, :].sum() + M[:, j].sum()
        scores[j - 1] = 2. * M[j, j] / den if den else 0.
        support[j - 1] = M[j, :].sum()
    av = float(np.sum(scores * support) / support.sum()) if support.sum() else 0.
    return scores, av


def eval_metrics(model, sess, dat_gen, iters=50, update=True, alt_attr=None):
    """`iters` batches of `dat_gen()` -> (batch_X, one-hot batch_mask [b, *spatial, c]) through the model; the metrics named
    by the keys of `model.valid_metrics` (or of the attribute `alt_attr`): 'acc' / 'av_acc' (voxel accuracy), 'F1' (binary, or
    the weighted multi-class score) and 'av_loss' (batch-size-weighted mean of model.loss).  update=True appends one value
    per metric to its list; otherwise the running results are returned."""
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
        results['accs'] = float(np.sum(preds == masks)) / preds.size
        results['F1s'] = binary_F1_score(preds, masks) if C == 2 else multi_F1_score(preds, masks, C)[1]
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
