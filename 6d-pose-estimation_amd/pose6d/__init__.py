"""pose6d — MI355X-native runtime for the SFR-Vision/6d-pose-estimation hot path.

Layers:
  _lib      ctypes binding of libpose6d.so (C ABI in include/pose6d.h)
  ops       torch.autograd.Functions over the C ABI (no CPU fallback)
  trunk     ResNet50 trunk engine: NHWC activations, packed weights, fused BN
  train     whole-step trainer (fwd + loss + bwd + clip + AdamW), hipGraph-captured
  validate  the epoch's validation pass on the trainer's engines (ADD metrics kept on the
            device until the epoch ends) and the plateau lr schedule
  store     device-resident frame store + epoch feeder (index-gathered training crops)
  infer     detection-to-pose inference: detector boxes -> crops -> eval forward -> projected
            3D boxes, one hipGraph per detection-count bucket
  ddp       batch-sharded data parallel over RCCL
The drop-in reference API lives in ../models (same module/class names).
"""
from ._lib import Pose6dError, load  # noqa: F401
from .infer import DEFAULT_K, CropDetections, PoseEstimator, load_mesh_corners  # noqa: F401
