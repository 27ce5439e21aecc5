"""cilrs_mi355 -- MI355X-native engine behind the reference's CILRS nn.Module boundary
(model/autonomous_drive.py:361-399, notebook/notebook.ipynb:440-555)."""
from .adversarial import GOALS as ADVERSARIAL_GOALS  # noqa: F401
from .adversarial import Attack as AdversarialAttack  # noqa: F401
from .bn_estimate import BatchNormEstimator, update_bn  # noqa: F401
from .cluster import Clustering  # noqa: F401
from .data import (WEATHER_CONDITIONS, BatchLoader, CachedBatchLoader, CameraModel,  # noqa: F401
                   DeviceDataset, ViewShift, WeatherMix, view_records, view_u8, weather_condition,
                   weather_u8)
from .model import CILRS, CILRSResNet50  # noqa: F401
from .neighbours import NeighbourIndex  # noqa: F401
from .priority import PrioritizedBatchLoader, PrioritySampler  # noqa: F401
from .select import FramePool, Selection  # noqa: F401
from .train import CONFIG_A, CONFIG_B, LOSS_KEYS, TrainConfig, Trainer  # noqa: F401
