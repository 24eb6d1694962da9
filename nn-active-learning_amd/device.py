"""Device context ("session") and device model behind the reference's `sess` / `model` pair.

The reference hands every query function a `tf.Session` and a `CNN` object and reaches the
device through `sess.run(getattr(model, var), feed_dict)` (PW_NN.py:466,522).  Here `sess` is a
`DeviceSession` (one HIP stream on one MI355X, a libalq context) and `model` a `DeviceModel`
(a libalq model: weights + activation workspace resident in HBM).  PyTorch-ROCm is used only
for device memory, the stream and (in pool_shard.py) torch.distributed.
This module is the import point; the code lives by concern in the device_*.py modules beside it."""
from ._lib import ALQ_CONV, ALQ_CONVT, ALQ_FC, ALQ_POOL, LayerT, LossT, check  # noqa: F401
from .device_host import Handle, LazyVarDict, MethodHandle, onehot_to_labels, out_map_shape, tf_param_shapes, translate_layers  # noqa: F401
from .device_model import DeviceModel  # noqa: F401
from .device_session import DeviceSession, default_session  # noqa: F401
