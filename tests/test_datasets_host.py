"""nnal_amd.datasets without a GPU: the NumPy path against the arrays the reference's own modules produced
(tests/golden/datasets.npz), the documented deviation for odd depths and 2-D batches, the mask -> class-id mapping,
DeviceLabels as a host array, the window check of alq_slice_batch (a host function of the library), and the bookkeeping of
get_dat_for_FT / combine_with_other_data on NumPy and on resident (here: CPU tensor) subjects."""
import numpy as np
import pytest

import nnal_amd  # noqa: F401
from nnal_amd import datasets
from nnal_amd.datasets import data_holders, utils
from tests import datasets_cases as cases
from tests.fake_device import FakeSession


@pytest.fixture(scope='module')
def g():
    return cases.golden()


# ------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize('tag,n_labeled', [('all', None), ('fixed', 1)])
def test_index_batches_equal_the_reference(g, tag, n_labeled):
    np.random.seed(int(g['mix_%s_seed' % tag]))
    gen = utils.gen_minibatch_labeled_unlabeled_inds(g['mix_L_indic'], 3, n_labeled)
    for k in range(9):
        parts = next(gen)
        assert np.array_equal(np.concatenate(parts), g['mix_%s_%d' % (tag, k)])
        assert [len(p) for p in parts] == list(g['mix_%s_%d_parts' % (tag, k)])
    assert np.random.rand() == float(g['mix_%s_after' % tag])


def test_luv_split_by_sizes_equals_the_reference(g):
    dat = cases.holder(data_holders.regular, [int(v) for v in g['luv_sizes']], seed=int(g['luv_seed']), load=False)
    for name in ('labeled_inds', 'unlabeled_inds', 'train_inds', 'valid_inds', 'test_inds', 'L_indic'):
        assert np.array_equal(np.asarray(getattr(dat, name)), g['luv_' + name]), name
    assert dat.tr_mask_paths == [dat.mask_addrs[i] for i in dat.train_inds] and dat.C == 3


def test_global2local_inds_equals_the_reference(g):
    out = utils.global2local_inds(g['g2l_inds'], list(g['g2l_sizes']))
    assert len(out) == len(g['g2l_sizes'])
    for i, l in enumerate(out):
        assert np.array_equal(l, g['g2l_out_%d' % i])


def test_d3_training_batches_equal_the_reference(g):
    d3 = cases.holder(data_holders.D3, cases.d3_luv())
    np.random.seed(int(g['d3_seed']))
    d3.create_train_valid_gens(4, [8, 8, 2], n_labeled_train=2)
    assert d3.train_n_slices == list(g['d3_train_n_slices']) and np.array_equal(d3.slices_L_indic, g['d3_slices_L_indic'])
    for k in range(int(g['d3_batches'])):
        X, Y = d3.train_gen_fn()
        assert X.dtype == np.float64 and Y.dtype == np.float64
        assert np.array_equal(X, g['d3_X_%d' % k]) and np.array_equal(Y, g['d3_Y_%d' % k]), k
    assert np.random.rand() == float(g['d3_after'])


def _pb_inputs():
    table, img_addrs, _ = cases.subjects()
    imgs = [[table[img_addrs[mod][s]] for mod in cases.MODS] for s in (0, 2)]
    return imgs, [table['/synthetic/sub0_mask'], table['/synthetic/sub2_mask']]


def test_prepare_batch_listed_slices_full_crop_equals_the_reference(g):
    imgs, masks = _pb_inputs()
    np.random.seed(31)
    X, Y = utils.prepare_batch_BrVol(imgs, masks, [12, 10, 2], 3, [3, 5], np.array([1, 0]))
    assert np.array_equal(X, g['pb_X']) and np.array_equal(Y, g['pb_Y'])
    assert np.random.rand() == float(g['pb_after'])          # crop == the full slice: nothing drawn
    _, Yn = utils.prepare_batch_BrVol(imgs, masks, [12, 10, 2], None, [3, 5], np.array([1, 0]))
    assert np.array_equal(Yn, g['pb_Y_nohot'], equal_nan=True)


# ------------------------------------------------------------------------------------------ the deviation
def test_2d_batch_is_plane_one_of_the_depth_two_batch():
    """a 2-D batch is the chosen slice itself - plane jz = 1 (offset 0) of the [h, w, 2] batch with the
    same draws; the reference returns zeros there and draws no crop."""
    imgs, masks = _pb_inputs()
    L = np.array([1, 0])
    np.random.seed(5)
    X3, Y3 = utils.prepare_batch_BrVol(imgs, masks, [8, 7, 2], 3, [3, 5], L)
    after3 = np.random.rand()
    np.random.seed(5)
    X2, Y2 = utils.prepare_batch_BrVol(imgs, masks, [8, 7], 3, [3, 5], L)
    assert np.random.rand() == after3                         # one crop draw per sample either way
    assert X2.shape == (2, 8, 7, 2) and Y2.shape == (2, 8, 7, 3)
    assert np.array_equal(X2, X3[:, 1]) and np.array_equal(Y2, Y3[:, 1])
    assert np.abs(X2).sum() > 0 and Y2[0].sum() > 0 and Y2[1].sum() == 0


def test_odd_depth_fills_every_plane():
    imgs, masks = _pb_inputs()
    np.random.seed(6)
    X, Y = utils.prepare_batch_BrVol(imgs, masks, [12, 10, 3], None, [1, 5], None)
    assert X.shape == (2, 3, 12, 10, 2)
    for i, zc in enumerate([1, 5]):
        for jz in range(3):
            for jm in range(2):
                assert np.array_equal(X[i, jz, :, :, jm], imgs[i][jm][:, :, zc - 1 + jz])
            assert np.array_equal(Y[i, jz], masks[i][:, :, zc - 1 + jz])
    # both ends of the window: the first and the last centre that fit
    utils.prepare_batch_BrVol(imgs, masks, [12, 10, 3], None, [1, 5], None)
    for bad in ([0, 5], [1, 6]):
        with pytest.raises(ValueError):
            utils.prepare_batch_BrVol(imgs, masks, [12, 10, 3], None, bad, None)
    with pytest.raises(ValueError):                              # even depth: planes zc - 1, zc
        utils.prepare_batch_BrVol(imgs, masks, [12, 10, 2], None, [0, 5], None)


def test_random_crop_never_draws_the_last_offset():
    img = np.arange(6 * 5).reshape(6, 5)
    np.random.seed(0)
    offs = {utils.random_crop(img, 4, 5)[1:] for _ in range(200)}
    assert offs == {(0, 0), (1, 0)}                              # randint(0, 6 - 4): offset 2 is never drawn; w fits: no draw
    c, h0, w0 = utils.random_crop(img, 2, 2, 3, 1)
    assert (h0, w0) == (3, 1) and np.array_equal(c, img[3:5, 1:3])


# ------------------------------------------------------------------------------------------ masks and labels
def test_mask_class_ids():
    mask = np.array([[0., 1., 2., 3.], [1.5, np.nan, -1., 7.]])
    assert utils.mask_class_ids(mask, np.arange(3)).tolist() == [[0, 1, 2, 255], [255, 255, 255, 255]]
    # mapped labels, as read_mask: 10 -> 0, 20 -> 1, 30 -> 2, anything else class 0
    mask = np.array([[10, 20, 30], [0, 25, 20]])
    ids = utils.mask_class_ids(mask, [10, 20, 30], mapped=True)
    assert ids.dtype == np.uint8 and ids.tolist() == [[0, 1, 2], [0, 0, 1]]
    table = {'m': mask}
    dat = data_holders.regular({'T1': ['a']}, ['m'], lambda p: table[p], None, [np.array([0]), np.array([], dtype=int), np.array([], dtype=int)],
                               [10, 20, 30])
    assert np.array_equal(dat.read_mask('m'), ids) and dat.read_mask('m').dtype == np.float64
    ident = data_holders.regular({'T1': ['a']}, ['m'], lambda p: table[p], None, [np.array([0]), np.array([], dtype=int), np.array([], dtype=int)],
                                 np.arange(3))
    assert ident.read_mask('m') is mask
    with pytest.raises(ValueError):
        utils.mask_class_ids(mask, np.arange(255))


def test_device_labels_as_array_is_the_numpy_one_hot(g):
    import torch
    imgs, masks = _pb_inputs()
    np.random.seed(8)
    _, Y = utils.prepare_batch_BrVol(imgs, masks, [8, 8, 2], 3, [3, 5], np.array([1, 0]))
    np.random.seed(8)
    rows = utils._draw_windows([m.shape for m in masks], 8, 8, [3, 5])
    ids = [utils.mask_class_ids(m, np.arange(3)) for m in masks]
    lab = np.stack([ids[i][h0:h0 + 8, w0:w0 + 8, zc - 1:zc + 1].transpose(2, 0, 1).astype(np.int32) for i, (zc, h0, w0) in enumerate(rows)])
    lab[1] = -1                   # the unlabelled sample
    lab[lab >= 3] = -1            # the bytes that are no class
    dl = datasets.DeviceLabels(torch.as_tensor(lab), 3, cases.counts_of(lab, 3))
    assert dl.shape == Y.shape and len(dl) == 2 and dl.ndim == 5
    A = np.asarray(dl)
    assert A.dtype == np.float64 and np.array_equal(A, Y)
    assert np.array_equal(np.argmax(dl, axis=-1), np.argmax(Y, axis=-1))          # as eval_metrics reads it
    assert np.asarray(dl, dtype=np.float32).dtype == np.float32
    assert dl.counts.sum() == lab.size and dl.counts[3] >= lab[1].size


# ------------------------------------------------------------------------------------------ the window check
def test_window_check_rejects_every_kind_of_bad_window():
    dims = [(12, 10, 6), (9, 11, 8)]
    crop = (2, 8, 8)          # z, h, w
    ok = [(0, 1, 4, 2, 1), (1, 7, 1, 3, 0), (0, 5, 0, 0, 1)]
    utils.check_windows(dims, ok, crop, 3)
    bad = {
        'subject above the range': (2, 1, 0, 0, 1),
        'negative subject': (-1, 1, 0, 0, 1),
        'window starts before plane 0': (0, 0, 0, 0, 1),
        'window ends after the last plane': (0, 6, 0, 0, 1),
        'negative slice': (0, -3, 0, 0, 1),
        'h0 + h > H': (0, 1, 5, 0, 1),
        'w0 + w > W': (0, 1, 0, 3, 1),
        'negative h0': (0, 1, -1, 0, 1),
        'negative w0': (1, 1, 0, -1, 1),
        'labelled flag': (0, 1, 0, 0, 2),
    }
    for why, d in bad.items():
        for pos in (0, 1):          # first or last of the batch
            desc = [d] + ok if pos == 0 else ok + [d]
            with pytest.raises(ValueError):
                utils.check_windows(dims, desc, crop, 3)
                pytest.fail(why)
    for C in (0, 255, -1):
        with pytest.raises(ValueError):
            utils.check_windows(dims, ok, crop, C)
    utils.check_windows(dims, ok, crop, 254)
    for c in ((0, 8, 8), (2, 0, 8), (2, 8, -1), (2, 13, 8)):
        with pytest.raises(ValueError):
            utils.check_windows(dims, ok, c, 3)
    utils.check_windows(dims, [(0, 0, 0, 0, 1), (0, 5, 4, 2, 1)], (1, 8, 8), 3)      # z = 1: every plane is a centre
    with pytest.raises(ValueError):
        utils.check_windows(dims, [(0, 6, 0, 0, 1)], (1, 8, 8), 3)
    utils.check_windows(dims, [(1, 1, 0, 0, 1), (1, 6, 1, 3, 1)], (3, 8, 8), 3)      # odd depth: planes zc - 1 .. zc + 1
    with pytest.raises(ValueError):
        utils.check_windows(dims, [(1, 7, 0, 0, 1)], (3, 8, 8), 3)


# ------------------------------------------------------------------------------------------ bookkeeping
def _resident(dat):
    """The loaded NumPy subjects of `dat` as resident ones on CPU tensors (the layout alq_vol_pack writes)."""
    import torch
    sess = FakeSession()

    def conv(imgs, mask):
        vol = torch.as_tensor(np.stack([np.asarray(v).transpose(2, 0, 1) for v in imgs], -1).astype(np.float32))
        ids = torch.as_tensor(np.ascontiguousarray(utils.mask_class_ids(mask, np.arange(dat.C)).transpose(2, 0, 1)))
        s = utils.ResidentSubject(sess, vol, ids)
        return s.imgs, s.mask_view
    for part in ('tr', 'val'):
        pairs = [conv(i, m) for i, m in zip(getattr(dat, part + '_imgs'), getattr(dat, part + '_masks'))]
        setattr(dat, part + '_imgs', [p[0] for p in pairs])
        setattr(dat, part + '_masks', [p[1] for p in pairs])
    return dat


@pytest.mark.parametrize('resident', [False, True])
def test_get_dat_for_FT(resident):
    luv = [np.array([0]), np.array([1, 2]), np.array([3])]
    table, img_addrs, mask_addrs = cases.subjects()
    mask_addrs[3] = '/synthetic/sub3_mask'
    dat = data_holders.regular(img_addrs, mask_addrs, lambda p: table[p], None, luv, np.arange(3))
    dat.load_images()
    ref_imgs, ref_masks = dat.tr_imgs, dat.tr_masks
    if resident:
        dat = _resident(dat)
    q = [np.array([4, 1]), np.array([], dtype=int)]
    new = data_holders.get_dat_for_FT(dat, q, keep_unlabeled=True)
    assert len(new.tr_imgs) == 3 and len(new.tr_masks) == 3 and list(new.L_indic) == [1., 1., 0.]
    assert new.tr_imgs[0] is dat.tr_imgs[0] and new.val_imgs is dat.val_imgs and new.val_masks is dat.val_masks
    assert new.tr_masks[1].shape == (9, 11, 2) and new.tr_masks[2].shape == (9, 11, 6) and len(new.tr_imgs[1]) == 2
    rest = np.delete(np.arange(8), q[0])
    if resident:
        for got, sel in ((new.tr_masks[1].subject, q[0]), (new.tr_masks[2].subject, rest)):
            want = np.stack([v[:, :, sel].transpose(2, 0, 1) for v in ref_imgs[1]], -1).astype(np.float32)
            assert np.array_equal(got.vol.numpy(), want)
            assert np.array_equal(got.mask.numpy(), utils.mask_class_ids(ref_masks[1][:, :, sel], np.arange(3)).transpose(2, 0, 1))
    else:
        for jm in range(2):
            assert np.array_equal(new.tr_imgs[1][jm], ref_imgs[1][jm][:, :, q[0]])
            assert np.array_equal(new.tr_imgs[2][jm], ref_imgs[1][jm][:, :, rest])
        assert np.array_equal(new.tr_masks[1], ref_masks[1][:, :, q[0]]) and np.array_equal(new.tr_masks[2], ref_masks[1][:, :, rest])
    lean = data_holders.get_dat_for_FT(dat, q)
    assert len(lean.tr_imgs) == 2 and list(lean.L_indic) == [1., 1.]
    with pytest.raises(AssertionError):
        data_holders.get_dat_for_FT(dat, q[:1])
    # the new object generates batches: every slice of its subjects is a training slice
    if not resident:
        lean.create_train_valid_gens(3, [8, 8])
        assert lean.train_n_slices == [6, 2]
        X, Y = lean.train_gen_fn()
        assert X.shape == (3, 8, 8, 2) and Y.shape == (3, 8, 8, 3)


def test_combine_with_other_data():
    a = cases.holder(data_holders.regular, [np.array([0]), np.array([1]), np.array([2])])
    b = cases.holder(data_holders.regular, [np.array([3, 0]), np.array([], dtype=int), np.array([1])])
    n_a = len(a.combined_paths)
    tr_a, tr_b = list(a.tr_img_paths), list(b.tr_img_paths)
    a.combine_with_other_data(b)
    assert list(a.train_inds) == [0, 1, 3 + n_a, 0 + n_a] and list(a.valid_inds) == [2, 1 + n_a] and list(a.test_inds) == [3, 2 + n_a]
    assert list(a.L_indic) == [1, 0, 1, 1] and len(a.combined_paths) == 2 * n_a and len(a.mask_addrs) == 2 * n_a
    assert a.tr_img_paths == tr_a + tr_b and len(a.tr_imgs) == 4 and len(a.tr_masks) == 4 and len(a.val_imgs) == 2
    assert all(len(v) == 2 * n_a for v in a.img_addrs.values())
    a.create_train_valid_gens(4, [8, 8, 2], valid_mode='full')
    assert a.train_n_slices == [6, 8, 6, 6] and a.valid_n_slices == [7, 8]
    other = cases.holder(data_holders.regular, [np.array([0]), np.array([1]), np.array([2])], load=False)
    other.mods = ['T1']
    with pytest.raises(AssertionError):
        a.combine_with_other_data(other)


def test_regular_generators_on_numpy_subjects():
    dat = cases.holder(data_holders.regular, [np.array([0, 1]), np.array([2]), np.array([1, 0])])
    np.random.seed(3)
    dat.create_train_valid_gens(4, [8, 8], valid_mode='random', n_labeled_train=None)
    X, Y = dat.train_gen_fn()
    assert X.shape == (4, 8, 8, 2) and Y.shape == (4, 8, 8, 3) and dat.train_n_slices == [6, 8, 7]
    Xv, Yv = dat.valid_gen_fn()
    assert Xv.shape == (2, 8, 8, 2) and Yv.sum() > 0
    dat.create_train_valid_gens(5, [8, 8], valid_mode='full')
    Xv, Yv = dat.valid_gen_fn()
    assert Xv.shape == (5, 8, 8, 2) and dat.valid_n_slices == [8, 6]


# ------------------------------------------------------------------------------------------ refusals
def test_refusals():
    imgs, masks = _pb_inputs()
    with pytest.raises(NotImplementedError):
        utils.prepare_batch_BrVol(imgs, masks, [8, 8], 3, 'non-uniform')
    with pytest.raises(ValueError):
        utils.prepare_batch_BrVol(imgs, masks, [8, 8], 3, 'sometimes')
    try:
        import nibabel  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError):
            utils.nii_reader('/nowhere.nii')
    with pytest.raises(ValueError):                              # a crop larger than the slice: the reference's randint refuses it too
        utils.prepare_batch_BrVol(imgs, masks, [13, 10], 3, [3, 5])
    dat = _resident(cases.holder(data_holders.regular, [np.array([0]), np.array([1]), np.array([], dtype=int)]))
    with pytest.raises(ValueError):                              # resident masks are class ids: the class count is needed
        utils.prepare_batch_BrVol(dat.tr_imgs, dat.tr_masks, [8, 8], None, [1, 1])
    with pytest.raises(AssertionError):
        cases.holder(data_holders.D3, cases.d3_luv()).create_train_valid_gens(4, [8, 8])
    assert not hasattr(utils, 'lesion_patch_gen')
