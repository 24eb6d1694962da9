"""Lesions of a binary mask as ranked connected components (reference: datasets/lesion_utils.py): `find_lesion_components`
numbers the components 1 .. K by descending volume, `drop_lesions_with_threshold` removes the ones below a volume.  Signatures
as in the reference, plus `sess` (the device session, default device.default_session()) and `shape`, with the conventions of
post_processing.py: an array in -> an array out (float64 ranks as the reference's np.zeros volume, np.uint8 for the
thresholded mask); a uint8 device tensor plus its `shape` in -> a device tensor out (int32 ranks, uint8 mask).

On the device (csrc/ccl.hip): alq_cc_label (26-connected; 8 for a 2-D mask) -> alq_cc_sizes -> the rank table -> alq_cc_relabel.
The table is built with torch over the K components, not over voxels: the roots, nonzero(sizes), come out ascending, which is
the order of each component's first voxel - skimage's label order - and a stable descending sort of their sizes gives the
ranks.  Equal volumes therefore go to the component that starts first in C order (the reference's np.argsort(-vols) leaves
ties open), the rule connected_component_analysis_3d documents.  Binary input only: another value raises ValueError.

mask[0, 0, 0] != 0 takes the host statement (`find_lesion_components_host`, on regions.cc_label_host): the reference then
reads that voxel's component as the background and ranks the zero set as a "lesion" of its own."""
import numpy as np


def find_lesion_components_host(mask):
    """lesion_utils.py:14-37 line by line, with regions.cc_label_host standing in for skimage.measure.label (labels 1 .. in the
    order of each component's first voxel, 0 = the zero voxels) and a stable argsort for the volume ties: float64 ranks."""
    from .. import regions
    mask = np.asarray(mask)
    lab = regions.cc_label_host(mask, 26)
    roots = np.unique(lab[lab >= 0])
    CC_labels = np.where(lab >= 0, np.searchsorted(roots, lab) + 1, 0)
    bkg_label = CC_labels.reshape(-1)[0]
    comp_labels = np.unique(CC_labels)
    comp_labels = comp_labels[comp_labels != bkg_label]
    vols = np.array([np.sum(CC_labels == i) for i in comp_labels])
    sorted_labels = comp_labels[np.argsort(-vols, kind='stable')] if len(comp_labels) else comp_labels
    new_CC_labels = np.zeros(CC_labels.shape)
    for i in range(len(sorted_labels)):
        new_CC_labels[CC_labels == sorted_labels[i]] = i + 1
    return new_CC_labels


def drop_lesions_with_threshold_host(mask, thr):
    """lesion_utils.py:40-53 on find_lesion_components_host: np.uint8 mask of the ranked components of at least `thr` voxels."""
    CC = find_lesion_components_host(mask)
    for label in np.unique(CC):
        vol = np.sum(CC == label)
        if vol < thr:
            CC[CC == label] = 0
    return np.uint8(CC > 0)


def _prepare(mask, sess, shape, name):
    """-> (session, uint8 device tensor or None, shape, came as an array, origin set, the host array or None)"""
    from .. import device
    sess = sess or device.default_session()
    torch = sess.torch
    if isinstance(mask, torch.Tensor):
        shape = tuple(int(v) for v in (tuple(mask.shape) if shape is None else shape))
        head = mask.reshape(-1)
        if int(head.numel()) and int(head.max()) > 1:
            raise ValueError('%s takes a binary mask (values 0 and 1)' % name)
        origin = bool(int(head[0]) != 0) if int(head.numel()) else False
        return sess, mask, shape, False, origin, None
    a = np.asarray(mask)
    if a.size and not np.all((a == 0) | (a == 1)):
        raise ValueError('%s takes a binary mask (values 0 and 1)' % name)
    origin = bool(a.reshape(-1)[0] != 0) if a.size else False
    d = None if origin else sess.to_device(a != 0, torch.uint8)
    return sess, d, a.shape, True, origin, a


def _labels_and_sizes(sess, d_mask, shape):
    labels = sess.cc_label(d_mask, shape, connectivity=26)
    return labels, sess.cc_sizes(labels)


def find_lesion_components(mask, sess=None, shape=None):
    """The connected components of a binary mask, re-indexed by volume: 1 on the largest lesion, 2 on the second largest, ...,
    0 on the background; equal volumes -> the component that starts first in C order."""
    sess, d_mask, shape, was_array, origin, a = _prepare(mask, sess, shape, 'find_lesion_components')
    torch = sess.torch
    if origin:
        host = find_lesion_components_host(a if was_array else d_mask.cpu().numpy().reshape(shape))
        return host if was_array else sess.to_device(host, torch.int32)
    labels, sizes = _labels_and_sizes(sess, d_mask, shape)
    flat = sizes.reshape(-1)
    roots = torch.nonzero(flat).reshape(-1)                              # ascending: the order of the components' first voxels
    order = torch.sort(flat[roots], descending=True, stable=True)[1]
    table = torch.zeros_like(flat)
    table[roots[order]] = torch.arange(1, int(roots.numel()) + 1, dtype=torch.int32, device=flat.device)
    ranks = sess.cc_relabel(labels, table=table.reshape(labels.shape))
    if was_array:
        return ranks.cpu().numpy().astype(np.float64).reshape(shape)
    return ranks.reshape(shape)


def drop_lesions_with_threshold(mask, thr, sess=None, shape=None):
    """The mask without the lesions (26-connected components) of fewer than `thr` voxels."""
    sess, d_mask, shape, was_array, origin, a = _prepare(mask, sess, shape, 'drop_lesions_with_threshold')
    torch = sess.torch
    if origin:
        host = drop_lesions_with_threshold_host(a if was_array else d_mask.cpu().numpy().reshape(shape), thr)
        return host if was_array else sess.to_device(host, torch.uint8)
    labels, sizes = _labels_and_sizes(sess, d_mask, shape)
    min_size = int(np.clip(np.ceil(thr), -2 ** 31, 2 ** 31 - 1))        # an integer size >= thr  <=>  >= ceil(thr)
    out = sess.cc_relabel(labels, sizes=sizes, min_size=min_size)
    if was_array:
        return out.cpu().numpy().astype(np.uint8).reshape(shape)
    return out.reshape(shape)
