"""Training on the GPU: the reference's epoch loop (training/trainer.py) with the batch supply, the NaN guard and the
per-type losses in HIP (csrc/trainer.hip), and the histograms of every parameter and gradient that
``wandb.watch`` shows of a run (csrc/watch.hip; section 4.26), and the per-feature firing counts that tell whether the
dictionary is alive (csrc/activity.hip; section 4.27), and the resampling step that revives its dead units from high-loss
rows (csrc/resample.hip; section 4.28), and the AuxK loss that gives them a gradient at every step (csrc/auxk.hip; section
4.29), and the nested-dictionary objective of the two top-k models (csrc/nested.hip; section 4.31), and BatchTopK, the
batch-wide selection they are trained with (csrc/batch_topk.hip; section 4.32), and JumpReLU, their per-unit learned thresholds
(csrc/jumprelu.hip; section 4.36)."""
from .auxk import aux_k_loss  # noqa: F401
from .nested import default_nested_bounds, nested_loss  # noqa: F401
from .multi_topk import default_multi_topk, multi_topk_loss  # noqa: F401
from .batch_topk import BatchTopK  # noqa: F401
from .jumprelu import JumpReLU  # noqa: F401
from .activity import ActivitySummary, FeatureActivity, activity_line  # noqa: F401
from .batches import EpochPlan, ShuffledChunk, epoch_permutation, plan_epoch  # noqa: F401
from .resample import ResampleReport, resample_dead  # noqa: F401
from .loss import RQ_STAGE_WEIGHTS, SAE_TYPES, recon_recipe, trainer_loss  # noqa: F401
from .trainer import Trainer, model_path_for  # noqa: F401
from .watch import WATCH_MODES, ModelWatch, TensorStats, tensor_stats  # noqa: F401

__all__ = ["Trainer", "ShuffledChunk", "EpochPlan", "epoch_permutation", "plan_epoch", "trainer_loss", "recon_recipe",
           "model_path_for", "SAE_TYPES", "RQ_STAGE_WEIGHTS", "ModelWatch", "TensorStats", "tensor_stats", "WATCH_MODES",
           "FeatureActivity", "ActivitySummary", "activity_line", "resample_dead", "ResampleReport", "aux_k_loss",
           "nested_loss", "default_nested_bounds", "BatchTopK",
           "multi_topk_loss", "default_multi_topk", "JumpReLU"]
