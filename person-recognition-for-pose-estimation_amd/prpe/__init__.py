"""prpe — MI355X-native (gfx950) per-frame inference hot path of the
Person-Recognition-for-Pose-Estimation combined multi-task model.

    from prpe import CombinedModel, TopDownPose, FrameIngest, non_max_suppression, keypoints_from_heatmaps

Device work: hand-written HIP kernels in ../csrc behind the C ABI of include/prpe.h
(libprpe.so, loaded by prpe._lib). PyTorch-ROCm supplies device memory, streams and
torch.distributed (RCCL) only.
"""
from .annotate import Annotator  # noqa: F401
from .arch import TASKS, state_dict_spec  # noqa: F401
from .clusters import FaceClustering, FaceClusters  # noqa: F401
from .evalsteps import CocoKeypointGT, PoseEvalStep, coco_keypoint_eval  # noqa: F401
from .faces import FaceCrops, PersonRecognition  # noqa: F401
from .gallery import FaceGallery, FaceIdentifier  # noqa: F401
from .identification import IdentificationEval  # noqa: F401
from .ingest import FrameIngest  # noqa: F401
from .model import CombinedModel, PoseOutput  # noqa: F401
from .nv12 import NV12Frames  # noqa: F401
from .postproc import keypoints_from_heatmaps, non_max_suppression, non_max_suppression_padded  # noqa: F401
from .topdown import TopDownPose  # noqa: F401
from .tracks import PersonTracker  # noqa: F401
from .verification import FaceVerification  # noqa: F401

__all__ = ["CombinedModel", "PoseOutput", "PoseEvalStep", "CocoKeypointGT", "coco_keypoint_eval",
           "TopDownPose", "FrameIngest", "NV12Frames", "FaceGallery", "FaceIdentifier", "FaceVerification",
           "IdentificationEval",
           "FaceClusters", "FaceClustering", "FaceCrops", "PersonRecognition", "PersonTracker", "Annotator",
           "non_max_suppression",
           "non_max_suppression_padded", "keypoints_from_heatmaps", "state_dict_spec", "TASKS"]
