"""`datasets/utils.py` of the reference: batch indices, the labelled / unlabelled mixture, the batch of slices or blocks cut
from loaded subjects (`prepare_batch_BrVol`) - on NumPy subjects the NumPy statement, on resident subjects
(`ResidentSubject`: packed once on the device by alq_vol_pack / alq_mask_pack) one alq_slice_batch call that leaves
`batch_X` and the labels on the device.  Both paths consume `np.random` draw for draw as the reference does: with one seed
they pick the same subjects, slices and crop offsets.

One deliberate deviation: plane jz of a sample is the slice at offset jz - z // 2 for EVERY depth
z.  The reference loops over `np.arange(-z_rad, z_rad)`, z_rad = int(z / 2): all z planes of an even depth (the same batch
as here), but the last plane of an odd depth stays zero and a 2-D `img_shape` (z = 1) gives an all-zero batch without a
crop draw.  Here an odd depth is filled and a 2-D batch is the slice itself, `random_crop` drawn once per sample as for any
other depth.  A window that leaves the volume along z (negative indices wrap in the reference) is a ValueError.

`lesion_patch_gen` (lesion tooling) and `slice_choice='non-uniform'` (the reference calls a `sample_pmf` whose import is
commented out) are not provided."""
import ctypes as C
from itertools import zip_longest

import numpy as np

NO_CLASS = 255          # the byte of a resident mask voxel that belongs to no class (an all-zero one-hot row)
_SRC_TYPES = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int16): 2, np.dtype(np.uint8): 3}


# ---------------------------------------------------------------------------------------------------------- indices
def gen_batch_inds(data_size, batch_size):
    """One random permutation of range(data_size) as a list of batches; the last one holds the remainder."""
    quot, rem = np.divmod(data_size, batch_size)
    perm = np.random.permutation(data_size).tolist()
    batches = [perm[i * batch_size:(i + 1) * batch_size] for i in range(quot)]
    if rem > 0:
        batches += [perm[-rem:]]
    return batches


def gen_minibatch_labeled_unlabeled_inds(L_indic, batch_size, n_labeled=None):
    """Endless generator of index tuples over a pool with the labelled indicator `L_indic`: 1-tuples of batches of the whole
    pool, or - with `n_labeled` - pairs (n_labeled labelled indices, batch_size - n_labeled unlabelled ones), each part
    re-permuted when it runs out."""
    n = len(L_indic)

    def eternal(pool, size):
        while True:
            for inds in gen_batch_inds(len(pool), size):
                yield pool[inds]

    if n_labeled is None:
        def whole():
            while True:
                for inds in gen_batch_inds(n, batch_size):
                    yield inds
        gens = (whole(),)
    else:
        labeled = np.where(L_indic == 1)[0]
        unlabeled = np.setdiff1d(np.arange(n), labeled)
        gens = (eternal(labeled, n_labeled), eternal(unlabeled, batch_size - n_labeled))
    return zip_longest(*gens)


def gen_minibatch_materials(gen, *args):
    inds = np.concatenate(next(gen))
    return tuple([[arg[ind] for ind in inds] for arg in args])


def global2local_inds(batch_inds, set_sizes):
    """Indices into the concatenation of ordered sets -> per set, the local indices that fall into it (in batch order)."""
    ends = np.append(-1, np.cumsum(set_sizes) - 1)
    which = ends.searchsorted(batch_inds) - 1
    return [np.array(batch_inds)[which == i] - ends[i] - 1 for i in range(len(set_sizes))]


def generator_complete_data(X, Y, batch_size, eternality=False, sample_axis=-1):
    """Batches (X part, Y part(s), indices) along `sample_axis` of one permutation, once or for ever."""
    batches = gen_batch_inds(X.shape[sample_axis], batch_size)
    sl = [slice(None)] * X.ndim
    while True:
        for batch in batches:
            sl[sample_axis] = batch
            if isinstance(Y, list):
                yield X[tuple(sl)], [y[tuple(sl)] for y in Y], batch
            else:
                yield X[tuple(sl)], Y[tuple(sl)], batch
        if not eternality:
            break


def nrrd_reader(path):
    from .. import nrrd_io
    return nrrd_io.read(path)[0]


def nii_reader(path):
    try:
        import nibabel as nib
    except ImportError:
        raise ImportError('nii_reader needs nibabel, which is not installed')
    return nib.load(path).get_data()


def random_crop(img, h, w, init_h=None, init_w=None):
    """(img[init_h:init_h + h, init_w:init_w + w], init_h, init_w); an offset not given is 0 where the axis fits exactly and
    `np.random.randint(0, size - h)` elsewhere - the reference's draw, which never returns the last offset size - h."""
    if init_h is None:
        init_h, init_w = _draw_crop(img.shape[0], img.shape[1], h, w)
    return img[init_h:init_h + h, init_w:init_w + w], init_h, init_w


def _draw_crop(H, W, h, w):
    init_h = 0 if H == h else np.random.randint(0, H - h)
    init_w = 0 if W == w else np.random.randint(0, W - w)
    return init_h, init_w


# ---------------------------------------------------------------------------------------------------------- resident subjects
class ResidentSubject(object):
    """A subject on the device: `vol` float32 [Z, H, W, m] (slice-major, modalities interleaved: the innermost order of
    batch_X) and `mask` uint8 [Z, H, W] of class ids (NO_CLASS: no class) or None.  `imgs` / `mask_view` are what
    `tr_imgs[i]` / `tr_masks[i]` hold: they answer len() and .shape as the reference's lists and arrays do."""

    def __init__(self, sess, vol, mask):
        self.sess, self.vol, self.mask = sess, vol, mask
        Z, H, W, m = (int(v) for v in vol.shape)
        self.shape, self.m = (H, W, Z), m
        self.imgs, self.mask_view = ResidentImages(self), ResidentMask(self)

    @classmethod
    def pack(cls, sess, imgs, mask_ids=None):
        """imgs: m host arrays [H, W, Z] of one shape (uploaded in their own dtype where the kernel reads it: float32, float64,
        int16, uint8; anything else as float64, which holds it exactly); mask_ids: uint8 [H, W, Z] class ids or None."""
        from .._lib import check, ptr
        torch = sess.torch
        imgs = [np.asarray(a) for a in imgs]
        shape = imgs[0].shape
        if len(shape) != 3 or any(a.shape != shape for a in imgs):
            raise ValueError('the modalities of a subject are 3-D arrays of one shape, got %r' % ([a.shape for a in imgs],))
        dt = imgs[0].dtype
        if dt not in _SRC_TYPES or any(a.dtype != dt for a in imgs):
            imgs, dt = [a.astype(np.float64) for a in imgs], np.dtype(np.float64)
        H, W, Z = shape
        dims = (C.c_int32 * 3)(H, W, Z)
        src = [torch.as_tensor(np.ascontiguousarray(a)).to(sess.device) for a in imgs]
        vol = sess.empty((Z, H, W, len(imgs)), torch.float32)
        sess.bind_stream()
        check(sess.lib.alq_vol_pack(sess.ctx, (C.c_void_p * len(src))(*[t.data_ptr() for t in src]), len(src), _SRC_TYPES[dt], dims,
                                    ptr(vol)))
        mask = None
        if mask_ids is not None:
            mask_ids = np.asarray(mask_ids)
            if mask_ids.dtype != np.uint8 or mask_ids.shape != shape:
                raise ValueError('class ids are uint8 %r, got %s %r' % (shape, mask_ids.dtype, mask_ids.shape))
            msrc = torch.as_tensor(np.ascontiguousarray(mask_ids)).to(sess.device)
            mask = sess.empty((Z, H, W), torch.uint8)
            check(sess.lib.alq_mask_pack(sess.ctx, ptr(msrc), dims, ptr(mask)))
        sess.synchronize()          # the unpacked copies go out of scope here
        return cls(sess, vol, mask)

    def take_slices(self, inds):
        """The subject of the slices `inds` (an index_select along the packed z axis): `img[:, :, inds]` of every modality."""
        idx = self.sess.to_device(np.asarray(inds, dtype=np.int64).reshape(-1), self.sess.torch.int64)
        return ResidentSubject(self.sess, self.vol.index_select(0, idx), None if self.mask is None else self.mask.index_select(0, idx))


class ResidentImages(object):
    def __init__(self, subject):
        self.subject = subject
        self.shape = subject.shape

    def __len__(self):
        return self.subject.m


class ResidentMask(object):
    def __init__(self, subject):
        self.subject = subject
        self.shape = subject.shape


def mask_class_ids(mask, class_labels, mapped=False):
    """A host mask as the bytes of a resident one.  mapped=False (`class_labels` is 0 .. C-1, the mask is read as it is): a
    value that is exactly one of 0 .. C-1 is its class, any other (fractions, NaN, labels outside) is NO_CLASS - the all-zero
    one-hot row the reference builds for it.  mapped=True (`read_mask` maps the file's labels): class c where the mask equals
    class_labels[c] (a later match wins, as in read_mask), class 0 everywhere else."""
    mask = np.asarray(mask)
    nC = len(class_labels)
    if not 1 <= nC <= 254:
        raise ValueError('%d classes (1 .. 254)' % nC)
    if mapped:
        ids = np.zeros(mask.shape, dtype=np.uint8)
        for c, label in enumerate(class_labels):
            ids[mask == label] = c
        return ids
    ids = np.full(mask.shape, NO_CLASS, dtype=np.uint8)
    for c in range(nC):
        ids[mask == c] = c
    return ids


class DeviceLabels(object):
    """`batch_Y` of a device batch: `labels` int32 [b, *spatial] on the device (-1: unlabelled voxel), the class count `C`
    and `counts` int64 [C + 1] on the host (voxels per class, the -1 voxels last).  np.asarray(.) is the float64 one-hot
    [b, *spatial, C] the reference would have fed, so host consumers (eval_utils.eval_metrics) work unchanged; a dense
    model's loss and train step read `labels` and `counts` and build no one-hot at all."""

    def __init__(self, labels, C, counts):
        self.labels, self.C = labels, int(C)
        self.counts = np.asarray(counts, dtype=np.int64).reshape(self.C + 1)
        self.shape = tuple(int(v) for v in labels.shape) + (self.C,)
        self.ndim = len(self.shape)

    def __len__(self):
        return self.shape[0]

    def __array__(self, dtype=None, copy=None):
        lab = self.labels.cpu().numpy()
        onehot = (lab[..., None] == np.arange(self.C)).astype(np.float64)
        return onehot if dtype is None else onehot.astype(dtype)


def check_windows(dims, desc, crop, C):
    """The host check of alq_slice_batch on its own (alq_slice_batch_check): ValueError with the library's message."""
    from .. import _lib
    dims = np.ascontiguousarray(dims, dtype=np.int32).reshape(-1, 3)
    desc = np.ascontiguousarray(desc, dtype=np.int32).reshape(-1, 5)
    crop = np.ascontiguousarray(crop, dtype=np.int32).reshape(3)
    i32 = C_i32
    rc = _lib.lib().alq_slice_batch_check(dims.ctypes.data_as(i32), len(dims), desc.ctypes.data_as(i32), len(desc), crop.ctypes.data_as(i32), int(C))
    if rc != 0:
        raise ValueError(_lib.lib().alq_last_error().decode())


C_i32 = C.POINTER(C.c_int32)


def slice_batch(sess, subjects, desc, crop, nclass, out=None):
    """alq_slice_batch: `subjects` ResidentSubject list, desc int [b][5] = (subject, zc, h0, w0, labelled), crop (z, h, w).
    Returns (X float32 [b, z, h, w, m], labels int32 [b, z, h, w], counts int64 [C + 1] on the DEVICE); a bad window is a
    ValueError before anything is launched."""
    from .._lib import ALQ_EINVAL, check, lib, ptr
    torch = sess.torch
    desc = np.ascontiguousarray(desc, dtype=np.int32).reshape(-1, 5)
    crop = np.ascontiguousarray(crop, dtype=np.int32).reshape(3)
    dims = np.ascontiguousarray([s.shape for s in subjects], dtype=np.int32).reshape(-1, 3)
    b, m = len(desc), subjects[0].m
    if any(s.m != m for s in subjects):
        raise ValueError('the subjects of a batch hold one number of modalities')
    z, h, w = (int(v) for v in crop)
    if out is None:
        out = (sess.empty((b, max(z, 0), max(h, 0), max(w, 0), m), torch.float32), sess.empty((b, max(z, 0), max(h, 0), max(w, 0)), torch.int32),
               sess.empty((max(int(nclass), 0) + 1,), torch.int64))
    X, lab, counts = out
    vols = (C.c_void_p * len(subjects))(*[s.vol.data_ptr() for s in subjects])
    masks = (C.c_void_p * len(subjects))(*[s.mask.data_ptr() if s.mask is not None else None for s in subjects])
    sess.bind_stream()
    rc = lib().alq_slice_batch(sess.ctx, vols, masks, dims.ctypes.data_as(C_i32), len(subjects), m, desc.ctypes.data_as(C_i32), b,
                               crop.ctypes.data_as(C_i32), int(nclass), ptr(X), ptr(lab), ptr(counts))
    if rc == ALQ_EINVAL:
        raise ValueError(lib().alq_last_error().decode())
    check(rc)
    return X, lab, counts


# ---------------------------------------------------------------------------------------------------------- the batch
def _crop_shape(img_shape):
    if len(img_shape) == 2:
        return int(img_shape[0]), int(img_shape[1]), 1
    h, w, z = img_shape
    return int(h), int(w), int(z)


def _draw_windows(shapes, h, w, slice_choice):
    """The draws of a batch in the reference's order - per sample the slice (uniform choice), then the crop offsets: rows
    (zc, h0, w0)."""
    if isinstance(slice_choice, str) and slice_choice != 'uniform':
        if slice_choice == 'non-uniform':
            raise NotImplementedError("slice_choice='non-uniform': the reference calls a sample_pmf whose import is commented out")
        raise ValueError('slice_choice %r' % (slice_choice,))
    rows = []
    for i, (H, W, Z) in enumerate(shapes):
        zc = np.random.randint(Z) if isinstance(slice_choice, str) else int(slice_choice[i])
        h0, w0 = _draw_crop(H, W, h, w)
        rows.append((zc, h0, w0))
    return rows


def prepare_batch_BrVol(imgs, masks, img_shape, one_hot_channels=None, slice_choice='uniform', labeled_indic=None):
    """A batch of b slices (`img_shape` = [h, w]) or blocks ([h, w, z]: planes zc - z // 2 .. zc - z // 2 + z - 1 around the
    chosen slice zc) out of b loaded subjects: imgs[i] the m modality arrays [H, W, Z] of sample i, masks[i] its mask.
    slice_choice: 'uniform' (one draw per sample) or the b slice indices; slices smaller than the subject are cropped at one
    random offset per sample.  labeled_indic[i] == 0: the sample is unlabelled (NaN mask; all-zero one-hot rows).
    Returns (batch_X float64 [b, z, h, w, m], batch_mask [b, z, h, w] or one-hot [b, z, h, w, one_hot_channels]), the depth
    axis squeezed when z = 1.  With resident subjects (imgs[i] / masks[i] of `ResidentSubject`) the same draws fill the
    descriptors of one alq_slice_batch call: (device float32 batch_X, DeviceLabels)."""
    b = len(imgs)
    h, w, z = _crop_shape(img_shape)
    if labeled_indic is None:
        labeled_indic = np.ones(b)
    resident = isinstance(masks[0], ResidentMask)
    if resident:
        return _prepare_batch_resident(imgs, masks, (h, w, z), one_hot_channels, slice_choice, labeled_indic)
    m = len(imgs[0])
    windows = _draw_windows([np.shape(masks[i]) for i in range(b)], h, w, slice_choice)
    batch_X = np.zeros((b, z, h, w, m))
    nohot = np.zeros((b, z, h, w))
    for i, (zc, h0, w0) in enumerate(windows):
        H, W, Z = np.shape(masks[i])
        zlo = zc - z // 2
        if zc < 0 or zlo < 0 or zlo + z > Z:
            raise ValueError('sample %d: planes %d .. %d leave the volume (%d planes)' % (i, zlo, zlo + z - 1, Z))
        for jm in range(m):
            batch_X[i, :, :, :, jm] = np.asarray(imgs[i][jm])[h0:h0 + h, w0:w0 + w, zlo:zlo + z].transpose(2, 0, 1)
        if labeled_indic[i] == 0:
            nohot[i] = np.nan
        else:
            nohot[i] = np.asarray(masks[i])[h0:h0 + h, w0:w0 + w, zlo:zlo + z].transpose(2, 0, 1)
    if one_hot_channels is not None:
        batch_mask = (nohot[..., None] == np.arange(one_hot_channels)).astype(np.float64)
    else:
        batch_mask = nohot
    if z == 1:
        batch_X, batch_mask = np.squeeze(batch_X, axis=1), np.squeeze(batch_mask, axis=1)
    return batch_X, batch_mask


def _prepare_batch_resident(imgs, masks, hwz, one_hot_channels, slice_choice, labeled_indic):
    h, w, z = hwz
    if one_hot_channels is None:
        raise ValueError('a resident batch carries class ids: one_hot_channels (the class count) is needed')
    subjects, index, desc = [], {}, []
    windows = _draw_windows([mk.shape for mk in masks], h, w, slice_choice)
    for i, (zc, h0, w0) in enumerate(windows):
        s = masks[i].subject
        if imgs[i].subject is not s:
            raise ValueError('sample %d: images and mask of different resident subjects' % i)
        if id(s) not in index:
            index[id(s)] = len(subjects)
            subjects.append(s)
        desc.append((index[id(s)], zc, h0, w0, 0 if labeled_indic[i] == 0 else 1))
    sess = subjects[0].sess
    X, lab, counts = slice_batch(sess, subjects, desc, (z, h, w), one_hot_channels)
    if z == 1:
        X, lab = X.squeeze(1), lab.squeeze(1)
    return X, DeviceLabels(lab, one_hot_channels, counts.cpu().numpy())
