"""MI355X-native cascade-classifier hot path (integral images + Haar/LBP window evaluation) behind the reference's
own plugin surface. The compute lives in cascadeclassifier_amd/csrc (HIP, gfx950) behind include/cascadeclassifier_amd.h."""
from ._lib import CascadeError, LIB_PATH  # noqa: F401
from .detector import (CascadeClassifier, frame_layout, group_rectangles, group_rectangles_device, resize_area,  # noqa: F401
                       scale_plan, to_gray)
from .evaluator import CascadeBoost, CvFeatureEvaluator, CvFeatureParams, NegativeMiner, device_exp  # noqa: F401
from .samples import (CvRNG, SampleParams, Sampler, create_samples_from_info, create_test_samples,  # noqa: F401
                      create_training_samples, read_info, samples_from_info, warp_perspective, write_info)
from .trainer import BackgroundReader, train_cascade  # noqa: F401
