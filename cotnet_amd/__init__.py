"""cotnet_amd -- MI355X-native implementation of CoTNet's CoT-block hot path.

Public surface mirrors the reference (JDAI-CV/CoTNet):
    cupy_layers.aggregation_zeropad      -> cotnet_amd.aggregation_zeropad  (LocalConvolution, aggregation_zeropad)
    cupy_layers.aggregation_zeropad_mix  -> cotnet_amd.aggregation_zeropad_mix
    models.cotnet                        -> cotnet_amd.cotnet               (CotLayer, CoXtLayer, Bottleneck, cotnet50 ...)
    models.cotnet_hybrid                 -> cotnet_amd.cotnet_hybrid        (CoTLayer, CoTBottleneck, se_cotnetd_* ...)
    models.lr_net                        -> cotnet_amd.lr_net               (SelfAttLayer, Bottleneck, lrnet50, lrnet50_ks3; lrnet50_k7 is this package's own)
    datasets.mixup (batch / elem / pair) -> cotnet_amd.mixup                (DeviceMixup, PerSampleMixup, create_mixup: host draw, device mixing)
    loss.cross_entropy                   -> cotnet_amd.loss                 (soft_target_cross_entropy, LabelSmoothingCrossEntropy)
    evaler.evaler / utils.meters         -> cotnet_amd.evaler               (Evaler, DeviceTestMeter, accuracy: scored on the device)
    models.factory / models.registry     -> cotnet_amd.registry             (create_model, register_model)
    models.features / features_only=True -> cotnet_amd.features             (FeatureInfo, FeatureListNet, FeatureDictNet: on the fused walker)
    utils.checkpoint_saver / models.helpers.resume_checkpoint -> cotnet_amd.checkpoint (CheckpointSaver, resume_checkpoint)
    optim.optim_factory / optim.adamw / optim.lookahead -> cotnet_amd.optim_factory (create_optimizer -> FlatSGD, FlatAdam, FlatAdamW;
                                            split_opt_name: `lookahead_*` -> the keywords lookahead_k, lookahead_alpha)
    scheduler (cosine_lr, tanh_lr, step_lr, plateau_lr, scheduler_factory) -> cotnet_amd.lr_schedule (CosineLRSchedule, TanhLRSchedule,
                                            StepLRSchedule, PlateauLRSchedule, create_scheduler -> (schedule, num_epochs))
    train.py (train_epoch, main) / utils.meters.TrainMeter -> cotnet_amd.trainer (ReplayedStep, TrainMeter, train_epoch, Trainer: the
                                            loop over one replayed step, no host read per step)
Device code lives in cotnet_amd/csrc (HIP, gfx950) behind the C ABI of include/cotnet_amd.h.
"""
from . import _lib  # noqa: F401
# NB: the functions `aggregation_zeropad` / `aggregation_zeropad_mix` are NOT re-exported here: they would shadow the
# sub-modules of the same name.  Import them from the sub-modules, as with the reference's cupy_layers package.
from . import aggregation_zeropad, aggregation_zeropad_mix  # noqa: F401
from .aggregation_zeropad import AggregationZeropad, LocalConvolution  # noqa: F401
from .aggregation_zeropad_mix import AggregationZeropadMix, LocalConvolutionMix  # noqa: F401
from .cotnet import Bottleneck, CotLayer, CoXtLayer, cotnet50, cotnet101, cotnext50_2x48d, cotnext101_2x48d  # noqa: F401
from .cotnet_hybrid import (CoTBottleneck, CoTHybridNet, CoTLayer, se_cotnetd_50, se_cotnetd_101,  # noqa: F401
                            se_cotnetd_152, se_cotnetd_152_L, se_cotnetd_200, se_cotnetd_270)
from . import local_relation  # noqa: F401  (the sub-module: import the functions from it, as with aggregation_zeropad)
from .lr_net import Bottleneck_K7, Bottleneck_Ks3, SelfAttLayer, lrnet50, lrnet50_k7, lrnet50_ks3  # noqa: F401
from .loss import LabelSmoothingCrossEntropy, MixedSoftTargetCrossEntropy, soft_target_cross_entropy  # noqa: F401
from .mixup import DeviceMixup, PerSampleMixup, create_mixup  # noqa: F401
from .evaler import DeviceTestMeter, Evaler, accuracy  # noqa: F401
from .registry import create_model, list_models, load_checkpoint, register_model  # noqa: F401
from .resnet import ResNet  # noqa: F401
from .features import FeatureDictNet, FeatureInfo, FeatureListNet  # noqa: F401
from .checkpoint import CheckpointSaver, resume_checkpoint  # noqa: F401
from .flat_adamw import FlatAdam, FlatAdamW  # noqa: F401
from .optim_factory import create_optimizer, split_opt_name  # noqa: F401
from .lr_schedule import (CosineLRSchedule, CosineSchedule, PlateauLRSchedule, StepLRSchedule, TanhLRSchedule,  # noqa: F401
                          create_scheduler)
from .trainer import ReplayedStep, TrainMeter, Trainer, train_epoch  # noqa: F401

__version__ = "0.1.0"
