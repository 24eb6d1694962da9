"""`datasets/data_holders.py` of the reference: `regular` (the labelled / unlabelled / validation split of a list of
subjects, their loading, the training and validation batch generators), `D3` (blocks of z slices) and `get_dat_for_FT`
(the data object of a fine-tuning round).  Attribute names, signatures and the consumption of `np.random` are the
reference's.

`load_images(sess)` with a device session keeps every subject RESIDENT (datasets.utils.ResidentSubject: uploaded in its file
dtype, packed once, the unpacked copy dropped); the generators then return `(device batch_X, DeviceLabels)` from one
launch per batch.  Without a session everything stays NumPy, as in the reference.  The site-specific `path_loader` and the
lesion tooling are not part of the package."""
import numpy as np

from .utils import (ResidentSubject, gen_minibatch_labeled_unlabeled_inds, gen_minibatch_materials, global2local_inds,
                    mask_class_ids, prepare_batch_BrVol)


class regular(object):

    def __init__(self, img_addrs, mask_addrs, data_reader, rnd_seed, LUV_inds_or_sizes, class_labels):
        """img_addrs {modality: [paths]}, mask_addrs [paths] ('NA': no mask), data_reader(path) -> array [H, W, Z].
        LUV_inds_or_sizes: [labelled, unlabelled, validation] as index arrays, or as sizes cut from one permutation seeded
        with rnd_seed; the subjects left over are the test set."""
        self.class_labels = class_labels
        self.C = len(self.class_labels)
        self.seed = rnd_seed
        self.reader = data_reader
        self.mask_reader = lambda x: self.read_mask(x)
        self.img_addrs = img_addrs
        self.mask_addrs = mask_addrs
        self.mods = list(img_addrs.keys())
        n = len(img_addrs[self.mods[0]])
        self.combined_paths = [[img_addrs[mod][i] for mod in self.mods] for i in range(n)]
        L, U, V = LUV_inds_or_sizes[:3]
        if isinstance(L, np.ndarray):
            self.labeled_inds, self.unlabeled_inds, self.valid_inds = L, U, V
            self.train_inds = np.concatenate((self.labeled_inds, self.unlabeled_inds))
        else:
            perm = np.random.RandomState(seed=rnd_seed).permutation(n)
            self.labeled_inds = perm[:L]
            self.unlabeled_inds = perm[L:L + U]
            self.train_inds = np.concatenate((self.labeled_inds, self.unlabeled_inds))
            self.valid_inds = perm[L + U:L + U + V]
        self.L_indic = np.array([1] * len(self.labeled_inds) + [0] * len(self.unlabeled_inds))
        self.test_inds = np.array(list(set(np.arange(n)) - set(self.train_inds) - set(self.valid_inds)))
        for part, inds in (('tr', self.train_inds), ('val', self.valid_inds), ('test', self.test_inds)):
            setattr(self, part + '_img_paths', [self.combined_paths[i] for i in inds])
            setattr(self, part + '_mask_paths', [self.mask_addrs[i] for i in inds])

    # -- loading -----------------------------------------------------------------------------------------------------
    def _identity_labels(self):
        return not np.any(np.asarray(self.class_labels) != np.arange(self.C))

    def read_mask(self, path):
        """The mask file with its labels mapped to 0 .. C-1 where `class_labels` is not already that range (float64,
        unmatched values 0); otherwise the file as it is."""
        orig = self.reader(path)
        if self._identity_labels():
            return orig
        mask = np.zeros(orig.shape)
        for c, label in enumerate(self.class_labels):
            mask[orig == label] = c
        return mask

    def _load_subject(self, img_paths, mask_path, sess):
        imgs = [self.reader(p) for p in img_paths]
        if sess is None:
            return imgs, (np.zeros(imgs[-1].shape) if mask_path == 'NA' else self.mask_reader(mask_path))
        if mask_path == 'NA':          # (an all-zero mask keeps the lists aligned; the subject should be unlabelled)
            ids = np.zeros(imgs[-1].shape, dtype=np.uint8)
        else:
            ids = mask_class_ids(self.reader(mask_path), self.class_labels, mapped=not self._identity_labels())
        s = ResidentSubject.pack(sess, imgs, ids)
        return s.imgs, s.mask_view

    def load_images(self, sess=None):
        """The training and validation subjects into `tr_imgs` / `tr_masks` / `val_imgs` / `val_masks`: lists of modality
        arrays and mask arrays, or - with a device session - of resident subjects."""
        self.tr_imgs, self.tr_masks, self.val_imgs, self.val_masks = [], [], [], []
        for paths, mpath in zip(self.tr_img_paths, self.tr_mask_paths):
            imgs, mask = self._load_subject(paths, mpath, sess)
            self.tr_imgs.append(imgs)
            self.tr_masks.append(mask)
        for paths, mpath in zip(self.val_img_paths, self.val_mask_paths):
            imgs, mask = self._load_subject(paths, mpath, sess)
            self.val_imgs.append(imgs)
            self.val_masks.append(mask)

    # -- generators --------------------------------------------------------------------------------------------------
    def _slice_margin(self, img_shape):
        return 0

    def _train_gens(self, batch_size, img_shape, n_labeled_train):
        margin = self._slice_margin(img_shape)
        self.train_n_slices = [mk.shape[2] - 2 * margin for mk in self.tr_masks]
        self.slices_L_indic = np.concatenate([np.ones(ns) * self.L_indic[i] for i, ns in enumerate(self.train_n_slices)])
        train_generator = gen_minibatch_labeled_unlabeled_inds(self.slices_L_indic, batch_size, n_labeled_train)
        self.train_gen_fn = lambda: self.generate_images(img_shape, train_generator, 'training')

    def create_train_valid_gens(self, batch_size, img_shape, valid_mode='random', n_labeled_train=None):
        """`train_gen_fn` (batches of slices drawn over all training slices; `n_labeled_train` fixes the labelled share) and
        `valid_gen_fn` ('random': subjects and slices drawn uniformly; 'full': as the training generator, over the
        validation slices).  Needs load_images()."""
        if len(self.tr_masks) > 0:
            self._train_gens(batch_size, img_shape, n_labeled_train)
        if len(self.val_masks) > 0:
            if valid_mode == 'random':
                valid_gen_inds = gen_minibatch_labeled_unlabeled_inds(np.ones(len(self.val_imgs)), batch_size)
                valid_gen = lambda: self.valid_generator(valid_gen_inds, img_shape, 'uniform')
            elif valid_mode == 'full':
                self.valid_n_slices = [mk.shape[2] for mk in self.val_masks]
                valid_slices_L_indic = np.concatenate([np.ones(ns) for ns in self.valid_n_slices])
                # (the reference stores the index generator under the method's name; the 'random' mode of this object is gone after)
                self.valid_generator = gen_minibatch_labeled_unlabeled_inds(valid_slices_L_indic, batch_size, None)
                valid_gen = lambda: self.generate_images(img_shape, self.valid_generator, 'validation')
            self.valid_gen_fn = valid_gen

    def generate_images(self, img_shape, inds_generator, mode='training'):
        inds = np.concatenate(next(inds_generator))
        training = mode == 'training'
        n_slices = self.train_n_slices if training else self.valid_n_slices
        local = global2local_inds(inds, n_slices)
        img_inds = np.concatenate([np.ones(len(l), dtype=int) * i for i, l in enumerate(local)])
        img_slice_inds = np.concatenate(local) + (self._slice_margin(img_shape) if training else 0)
        pool_imgs, pool_masks = (self.tr_imgs, self.tr_masks) if training else (self.val_imgs, self.val_masks)
        imgs = [pool_imgs[int(i)] for i in img_inds]
        masks = [pool_masks[int(i)] for i in img_inds]
        inds_L_indic = None
        if training and np.any(self.L_indic == 0):
            inds_L_indic = np.ones(len(img_inds))
            inds_L_indic[self.L_indic[img_inds] == 0] = 0
        return prepare_batch_BrVol(imgs, masks, img_shape, self.C, img_slice_inds, inds_L_indic)

    def valid_generator(self, generator, img_shape, slice_choice='uniform'):
        if hasattr(self, 'val_imgs'):
            imgs, masks = gen_minibatch_materials(generator, self.val_imgs, self.val_masks)
        else:
            imgs, masks = gen_minibatch_materials(generator, self.val_img_paths, self.val_mask_paths)
        return prepare_batch_BrVol(imgs, masks, img_shape, self.C, slice_choice)

    def combine_with_other_data(self, dat_2):
        assert self.mods == dat_2.mods, 'The combining data sets should have the same image modalities.'
        off = len(self.combined_paths)
        for mod in self.mods:
            self.img_addrs[mod] += dat_2.img_addrs[mod]
        self.mask_addrs += dat_2.mask_addrs
        self.L_indic = np.concatenate((self.L_indic, dat_2.L_indic))
        for name in ('train_inds', 'valid_inds', 'test_inds'):
            setattr(self, name, np.concatenate((getattr(self, name), getattr(dat_2, name) + off)))
        self.combined_paths += dat_2.combined_paths
        for part in ('tr', 'val', 'test'):
            for kind in ('_img_paths', '_mask_paths'):
                setattr(self, part + kind, getattr(self, part + kind) + getattr(dat_2, part + kind))
        if hasattr(self, 'tr_imgs') and hasattr(dat_2, 'tr_imgs'):
            for name in ('tr_imgs', 'tr_masks', 'val_imgs', 'val_masks'):
                setattr(self, name, getattr(self, name) + getattr(dat_2, name))


class D3(regular):
    """Training batches of blocks: `img_shape` = [h, w, z], batches [b, z, h, w, m]; z // 2 slices at either end of a subject
    are no block centres.  (As in the reference, this class builds the training generator only.)"""

    def _slice_margin(self, img_shape):
        return int(img_shape[2] / 2)

    def create_train_valid_gens(self, batch_size, img_shape, valid_mode='random', n_labeled_train=None):
        assert len(img_shape) == 3, 'Three values are needed for img_shape in this class'
        assert img_shape[0] % 2 == img_shape[1] % 2, 'Height and Width sizes in img_shape should have one parity.'
        if len(self.tr_masks) > 0:
            self._train_gens(batch_size, img_shape, n_labeled_train)


def _take(imgs, mask, inds):
    """`[img[:, :, inds] for img in imgs], mask[:, :, inds]` of a loaded subject, NumPy or resident."""
    if hasattr(mask, 'subject'):
        s = mask.subject.take_slices(inds)
        return s.imgs, s.mask_view
    return [img[:, :, inds] for img in imgs], mask[:, :, inds]


def get_dat_for_FT(dat, slice_img_inds, keep_unlabeled=False):
    """The data object of a fine-tuning round: slice_img_inds[i] are the queried slices of the i-th UNLABELLED training
    subject of `dat`; they join the labelled subjects with their true masks (one new subject per queried subject).  With
    keep_unlabeled the remaining slices of those subjects stay as unlabelled subjects.  Validation data are shared."""
    labeled_size = int(np.sum(dat.L_indic))
    assert len(slice_img_inds) == len(dat.tr_imgs[labeled_size:]), \
        'The list of queried slices and list of unlabeled images should have the same length.'
    new_dat = regular(dat.img_addrs, dat.mask_addrs, dat.reader, None, [dat.labeled_inds, dat.unlabeled_inds, dat.valid_inds],
                      dat.class_labels)
    L_imgs, L_masks = list(dat.tr_imgs[:labeled_size]), list(dat.tr_masks[:labeled_size])
    U_imgs, U_masks = [], []
    for i, q in enumerate(slice_img_inds):
        if len(q) == 0:
            continue
        imgs, mask = dat.tr_imgs[i + labeled_size], dat.tr_masks[i + labeled_size]
        a, b = _take(imgs, mask, q)
        L_imgs.append(a)
        L_masks.append(b)
        if keep_unlabeled:
            a, b = _take(imgs, mask, np.delete(np.arange(mask.shape[2]), q))
            U_imgs.append(a)
            U_masks.append(b)
    new_dat.tr_imgs, new_dat.tr_masks = L_imgs + U_imgs, L_masks + U_masks
    new_dat.L_indic = np.concatenate((np.ones(len(L_masks)), np.zeros(len(U_masks))))
    new_dat.val_imgs, new_dat.val_masks = dat.val_imgs, dat.val_masks
    return new_dat
