"""Post-processing, host side (no GPU): the scipy restatements regions.cc_label_host / keep_largest_host / fill_holes_host
against expected arrays written down from how the test volumes were built (tests/postproc_cases.py), and the origin / tie /
error logic of post_processing.connected_component_analysis_3d and fill_holes through a small session whose two device calls
are those restatements."""
import numpy as np
import pytest
import torch

import nnal_amd  # noqa: F401
from tests import postproc_cases as pc
from tests.fake_device import FakeSession


class HostPPSession(FakeSession):
    """FakeSession + the two post-processing calls of DeviceSession, computed by the host restatements."""

    def __init__(self):
        self.calls = []

    def cc_keep_largest(self, seg, shape, connectivity=26, skip_origin=True, out=None):
        from nnal_amd import regions
        assert seg.dtype == torch.uint8 and out is None
        self.calls.append(('cc', connectivity, skip_origin))
        mask, info = regions.keep_largest_host(seg.numpy().reshape(shape), connectivity, skip_origin, with_info=True)
        return torch.as_tensor(mask), info

    def fill_holes(self, seg, shape, out=None):
        from nnal_amd import regions
        assert seg.dtype == torch.uint8 and out is None
        self.calls.append(('fill',))
        mask, info = regions.fill_holes_host(seg.numpy().reshape(shape), with_info=True)
        return torch.as_tensor(mask), info


def test_label_host_on_built_shapes():
    from nnal_amd import regions
    for name, seg, expected in pc.built_label_cases():
        for conn in pc.CONNS:
            got = regions.cc_label_host(seg, conn)
            assert got.dtype == np.int32
            np.testing.assert_array_equal(got, expected[conn], err_msg='%s, connectivity %d' % (name, conn))


def test_label_host_polarity_and_2d():
    from nnal_amd import regions
    seg = np.ones((3, 4, 5), dtype=np.uint8)
    seg[1, 1, 1:4] = 0
    seg[2, 3, 4] = 0
    want = np.full(seg.shape, -1, dtype=np.int32)
    want[1, 1, 1:4] = np.ravel_multi_index((1, 1, 1), seg.shape)
    want[2, 3, 4] = seg.size - 1
    np.testing.assert_array_equal(regions.cc_label_host(seg, 26, select_zero=True), want)
    np.testing.assert_array_equal(regions.cc_label_host(seg, 6, select_zero=False), np.where(seg != 0, 0, -1))
    img = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0], [1, 1, 0]], dtype=np.uint8)
    np.testing.assert_array_equal(regions.cc_label_host(img, 6), [[0, -1, -1], [-1, 4, -1], [-1, -1, -1], [9, 9, -1]])
    np.testing.assert_array_equal(regions.cc_label_host(img, 18), [[0, -1, -1], [-1, 0, -1], [-1, -1, -1], [9, 9, -1]])


def test_keep_largest_host():
    from nnal_amd import regions
    seg = np.zeros((4, 5, 6), dtype=np.uint8)
    seg[0, 0, 0:2] = 1              # the origin's component, 2 voxels
    seg[1, 2, 1:4] = 1              # 3 voxels, first in C order
    seg[3, 4, 3:6] = 1              # 3 voxels
    seg[2, 0, 5] = 1
    first = np.zeros_like(seg)
    first[1, 2, 1:4] = 1
    mask, info = regions.keep_largest_host(seg, with_info=True)
    np.testing.assert_array_equal(mask, first)
    assert mask.dtype == np.uint8 and info.dtype == np.int64
    assert info.tolist() == [3, int(np.ravel_multi_index((1, 2, 1), seg.shape)), 3, 9]
    seg[0, 0, 2:4] = 1              # now the origin's component is the largest
    org = np.zeros_like(seg)
    org[0, 0, 0:4] = 1
    mask, info = regions.keep_largest_host(seg, skip_origin=False, with_info=True)
    np.testing.assert_array_equal(mask, org)
    assert info.tolist() == [4, 0, 4, 11]
    np.testing.assert_array_equal(regions.keep_largest_host(seg), first)
    mask, info = regions.keep_largest_host(org, with_info=True)                 # nothing but the origin's component
    assert not mask.any() and info.tolist() == [0, -1, 0, 4]
    # the issue's tie: the two largest components of this volume both have 8 voxels
    lab = pc.host_labels(pc.SMALL, 0.05, 26, False)
    roots, sizes = np.unique(lab[lab >= 0], return_counts=True)
    assert sorted(sizes)[-2:] == [8, 8]
    mask, info = regions.keep_largest_host(pc.random_volume(pc.SMALL, 0.05), with_info=True)
    assert info[1] == roots[sizes == 8].min() and info[2] == 8
    np.testing.assert_array_equal(mask, lab == info[1])


def test_fill_holes_host_on_built_shapes():
    from nnal_amd import regions
    for name, seg, want, info in pc.built_fill_cases():
        got, ginfo = regions.fill_holes_host(seg, with_info=True)
        assert got.dtype == np.uint8
        np.testing.assert_array_equal(got, want, err_msg=name)
        assert ginfo.tolist() == info, name
        np.testing.assert_array_equal(regions.fill_holes_host(seg), want)


def test_the_issue_volumes_are_what_the_issue_says():
    lab = pc.host_labels(pc.BOX, 0.05, 26, False)
    sizes = np.unique(lab[lab >= 0], return_counts=True)[1]
    assert len(sizes) == 708 and sizes.max() == 23
    lab = pc.host_labels(pc.BOX, 0.35, 26, False)
    assert np.unique(lab[lab >= 0], return_counts=True)[1].max() == 9710
    from nnal_amd import regions
    assert [int(regions.fill_holes_host(pc.fill_volume(pc.BOX, d), with_info=True)[1][1]) for d in pc.FILL_DENSITIES] == [793, 3913, 2072]


def test_wrapper_origin_and_tie_logic():
    from nnal_amd import post_processing as pp
    sess = HostPPSession()
    branches = set()
    for name, seg in pc.wrapper_cases():
        want = pc.reference_cca(seg)
        got = pp.connected_component_analysis_3d(seg, sess)
        assert got.dtype == np.uint32 and got.shape == seg.shape
        np.testing.assert_array_equal(got, want, err_msg=name)
        branches.add((bool(seg[0, 0, 0]), bool(np.array_equal(got, seg == 0))))
        # a device tensor plus its shape in, a device tensor out
        t = pp.connected_component_analysis_3d(torch.as_tensor(seg.reshape(-1)), sess, seg.shape)
        assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8
        np.testing.assert_array_equal(t.numpy().reshape(seg.shape), want)
    assert branches == {(False, False), (True, True), (True, False)}
    assert all(c == ('cc', 26, True) for c in sess.calls)
    # other number types in: the mask is what counts
    seg = pc.wrapper_cases()[0][1]
    np.testing.assert_array_equal(pp.connected_component_analysis_3d(seg.astype(np.float64), sess), pc.reference_cca(seg))


def test_wrapper_errors():
    from nnal_amd import post_processing as pp
    sess = HostPPSession()
    ones = np.ones((3, 4, 5), dtype=np.uint8)
    for seg in (ones, np.zeros((3, 4, 5), dtype=np.uint8)):
        with pytest.raises(IndexError):
            pc.reference_cca(seg)
        with pytest.raises(IndexError):
            pp.connected_component_analysis_3d(seg, sess)
    lone = np.zeros((3, 4, 5), dtype=np.uint8)
    lone[0, 0, 0:2] = 1                                     # the origin's component and zeros: the zero set is the answer
    np.testing.assert_array_equal(pp.connected_component_analysis_3d(lone, sess), lone == 0)
    np.testing.assert_array_equal(pc.reference_cca(lone), lone == 0)
    two = ones.copy()
    two[1, 1, 1] = 2
    with pytest.raises(ValueError):
        pp.connected_component_analysis_3d(two, sess)
    with pytest.raises(ValueError):
        pp.connected_component_analysis_3d(torch.as_tensor(two), sess, two.shape)
    with pytest.raises(ValueError):
        pp.fill_holes(np.zeros((4, 5), dtype=np.uint8), sess)


def test_fill_holes_wrapper():
    from nnal_amd import post_processing as pp
    sess = HostPPSession()
    for name, seg, want, _ in pc.built_fill_cases():
        got = pp.fill_holes(seg, sess)
        assert got.dtype == np.uint32
        np.testing.assert_array_equal(got, want, err_msg=name)
    seg = pc.built_fill_cases()[0][1]
    t = pp.fill_holes(torch.as_tensor(seg), sess)
    assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8
    np.testing.assert_array_equal(t.numpy(), pc.built_fill_cases()[0][2])
    np.testing.assert_array_equal(pp.fill_holes(seg.astype(bool), sess), pc.built_fill_cases()[0][2])


def test_full_model_eval_default_does_not_touch_the_new_calls():
    """post_process defaults to False and the argument comes last: existing callers are untouched."""
    import inspect
    from nnal_amd import PW_analyze_results as R
    sig = inspect.signature(R.full_model_eval)
    assert list(sig.parameters)[-2:] == ['save_dir', 'post_process'] and sig.parameters['post_process'].default is False


def test_symbols_and_build_lists():
    import os
    import re
    from nnal_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'alq.h')).read()
    for sym in ('alq_cc_work_bytes', 'alq_cc_label', 'alq_cc_keep_largest', 'alq_fill_holes'):
        assert re.search(r'\b%s\(' % sym, hdr) and sym in _lib.exported_names(), sym
    sh = open(os.path.join(root, 'nn-active-learning_amd', 'csrc', 'build.sh')).read()
    assert re.search(r'for f in [^;]*\bccl\b[^;]*; do', sh) and re.search(r'\{[a-z0-9,]*\bccl\b[a-z0-9,]*\}\.o', sh)
    _lib.build()
    dims = (_lib.C.c_int64 * 3)(21, 19, 70)
    assert _lib.lib().alq_cc_work_bytes(dims) == 64 + 8 * 21 * 19 * 70
    assert _lib.lib().alq_cc_work_bytes((_lib.C.c_int64 * 3)(2048, 2048, 512)) == 0       # 2^31 voxels
    assert _lib.lib().alq_cc_work_bytes((_lib.C.c_int64 * 3)(4, 0, 4)) == 0
