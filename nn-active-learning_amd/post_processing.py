"""Post-processing of a binary segmentation (reference: post_processing.py, applied by eval_utils.get_full_segs(...,
post_process=True)): `connected_component_analysis_3d` keeps the largest connected component, `fill_holes` fills the enclosed
cavities.  Signatures as in the reference, plus `sess` (the device session, default device.default_session()) and `shape`.

Both run on the device (csrc/ccl.hip: alq_cc_keep_largest, alq_fill_holes).  An array in -> np.uint32 out, as the reference
returns; a uint8 device tensor plus its `shape` in -> a uint8 device tensor out, nothing but 32 bytes of counts (and, for the
component analysis, the first voxel) crossing to the host.  The reference needs skimage.measure.label; its behaviour is
restated here from that function's documented defaults (regions.keep_largest_host / fill_holes_host are the host statements
the tests compare with)."""
import numpy as np


def _to_device(seg, sess, shape):
    """-> (session, uint8 device tensor, shape, came as an array)."""
    from . import device
    sess = sess or device.default_session()
    torch = sess.torch
    if isinstance(seg, torch.Tensor):
        if shape is None:
            shape = tuple(seg.shape)
        return sess, seg, tuple(int(v) for v in shape), False
    a = np.asarray(seg)
    return sess, sess.to_device(a != 0, torch.uint8), a.shape, True


def connected_component_analysis_3d(seg, sess=None, shape=None):
    """post_processing.py:8-35, literally:
      * skimage.measure.label(seg) at its defaults: full connectivity (26 neighbours in 3-D), value 0 is background label 0,
        only equal values connect.  Binary input only - a value outside {0, 1} raises ValueError (a deliberate deviation: the
        reference would label every value on its own; no caller passes anything but a binary mask);
      * the label at (0, 0, 0) leaves the candidates, and np.unique puts label 0 - all zero voxels as ONE set - among them.
        seg[0, 0, 0] == 0: the result is the largest foreground component.  seg[0, 0, 0] != 0: that voxel's component is out,
        and the zero set competes with the other foreground components; it wins ties (label 0 comes first), and then the
        result is the mask of the zero voxels;
      * no candidate at all: IndexError, as the reference's `[0]` on an empty argsort;
      * equal sizes (np.argsort(-vols)[0], implementation-defined there): the component that starts first in C order.
    The decision is taken from the 32 bytes alq_cc_keep_largest returns: zero voxels = nvox - info[3] against info[2]."""
    sess, d_seg, shape, was_array = _to_device(seg, sess, shape)
    torch = sess.torch
    if was_array:
        a = np.asarray(seg)
        if a.size and not np.all((a == 0) | (a == 1)):
            raise ValueError('connected_component_analysis_3d takes a binary mask (values 0 and 1)')
        origin = bool(a.reshape(-1)[0] != 0) if a.size else False
    else:
        head = d_seg.reshape(-1)
        if int(head.max()) > 1:
            raise ValueError('connected_component_analysis_3d takes a binary mask (values 0 and 1)')
        origin = bool(int(head[0]) != 0)
    out, info = sess.cc_keep_largest(d_seg, shape, connectivity=26, skip_origin=True)
    nvox = int(np.prod(shape))
    zeros = nvox - int(info[3])
    if origin and zeros > 0 and zeros >= int(info[2]):
        out = (d_seg == 0).to(torch.uint8).reshape(out.shape)        # label 0, the zero set, is the largest candidate
    elif int(info[1]) < 0:
        raise IndexError('index 0 is out of bounds for axis 0 with size 0')      # no candidate component
    if was_array:
        return out.cpu().numpy().astype(np.uint32).reshape(shape)
    return out


def fill_holes(seg, sess=None, shape=None):
    """post_processing.py:37-41: np.uint32(scipy.ndimage.binary_fill_holes(seg)) - every 6-connected set of zero voxels that
    reaches none of the six faces of the volume becomes 1.  3-D volumes only (a 2-D image has a different border rule in scipy
    than the one-slice volume the kernel would see)."""
    sess, d_seg, shape, was_array = _to_device(seg, sess, shape)
    if len(shape) != 3:
        raise ValueError('fill_holes takes a 3-D volume, not shape %r' % (shape,))
    out, _ = sess.fill_holes(d_seg, shape)
    if was_array:
        return out.cpu().numpy().astype(np.uint32).reshape(shape)
    return out
