"""The reference's `datasets` package: `data_holders` (regular, D3, get_dat_for_FT) and `utils` (batch indices,
prepare_batch_BrVol, ...), with subjects that can stay resident on the device (utils.ResidentSubject) and batches that
are built there (csrc/volbatch.hip): `(device batch_X, DeviceLabels)`; `lesion_utils` (lesions as ranked connected components,
csrc/ccl.hip)."""
from . import data_holders, lesion_utils, utils  # noqa: F401
from .data_holders import D3, get_dat_for_FT, regular  # noqa: F401
from .utils import DeviceLabels, ResidentSubject  # noqa: F401
