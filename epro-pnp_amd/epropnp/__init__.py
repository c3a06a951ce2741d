"""MI355X-native EPro-PnP layer.  Same import surface as the reference's `epropnp` package
(`from epropnp.epropnp import EProPnP6DoF`, ...); the LM solver and the AMIS sampler run as hand-written
HIP kernels behind a C ABI (include/epropnp_hip.h).  Beyond that surface: `epropnp.deform`, the detection head's deformable
attention sampler (the step that makes the correspondences) as one fused op and a drop-in module, and `epropnp.roi`, the cross-RoI
logsumexp / log-softmax / softmax of its auxiliary losses (the reference's `ops/inter_roi_ops.py`) and the RoIAlign that feeds them
(`roi_align`, `roi_align_wrapper`, `extract_rois`: the head's three `mmcv.ops.roi_align` calls).  Like `epropnp.boxes` and
`epropnp.metrics`, `epropnp.evaluation` (the KITTI AP evaluation: `kitti_eval`, `eval_class`, ...) and `epropnp.targets` (the training
step's centre targets, point targets and object sampling: `volume_centers`, `VolumeCenter`, `point_targets`, `get_targets`,
`obj_sampler`) are submodules imported by name."""
from . import deform  # noqa: F401,E402
from . import roi  # noqa: F401,E402
from .roi import logsoftmax_across_rois, logsumexp_across_rois, softmax_across_rois  # noqa: F401,E402
from .roi import extract_rois, roi_align, roi_align_wrapper  # noqa: F401,E402
