"""MI355X-native EPro-PnP layer.  Same import surface as the reference's `epropnp` package
(`from epropnp.epropnp import EProPnP6DoF`, ...); the LM solver and the AMIS sampler run as hand-written
HIP kernels behind a C ABI (include/epropnp_hip.h).  Beyond that surface: `epropnp.deform`, the detection head's deformable
attention sampler (the step that makes the correspondences) as one fused op and a drop-in module."""
from . import deform  # noqa: F401,E402
