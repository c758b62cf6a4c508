"""multimodal_mtrssm_amd -- MI355X-native MoPoE-M(MT)RSSM rollout path.

Drop-in classes for the hot path of Mamo1031/Multimodal-MTRSSM (``State`` / ``MTState``,
``Representation`` / ``Transition`` / ``MTRNN``, ``MoPoE_MRSSM`` / ``MoPoE_MMTRSSM``, ``likelihood``)
running on hand-written HIP kernels for gfx950 through the C-ABI of ``include/mtrssm.h``.
Importing the package does not need a GPU; running a rollout does, and fails loudly otherwise.
"""

from multimodal_mtrssm_amd.carry import StateCarry
from multimodal_mtrssm_amd.cnn import Decoder, Encoder
from multimodal_mtrssm_amd.core import MoPoE_MMTRSSM, MoPoE_MRSSM, WeightedMoPoE_MMTRSSM, WeightedMoPoE_MRSSM
from multimodal_mtrssm_amd.dataset import (
    DeviceEpisodeLoader,
    EpisodeBatch,
    EpisodeDataModule,
    EpisodeDataModuleConfig,
    FeedAugment,
    augment_key,
    feed_augment_parameters,
    feed_augment_reference,
)
from multimodal_mtrssm_amd.digit_train import DigitStats, DigitTrainer, dropout_mask_reference, tape_reference
from multimodal_mtrssm_amd.digits import DigitClassifier
from multimodal_mtrssm_amd.distributions import (
    Distribution,
    MultiOneHot,
    MultiOneHotFactory,
    cat_distribution,
    inject_uniforms,
    kl_divergence,
    stack_distribution,
)
from multimodal_mtrssm_amd.census import CensusTable, LatentCensus
from multimodal_mtrssm_amd.coherence import CoherenceTable, GenerationCoherence
from multimodal_mtrssm_amd.frechet import FrechetDistance, FrechetTable
from multimodal_mtrssm_amd.dropout import ModalityDropout
from multimodal_mtrssm_amd.experts import ExpertWeights
from multimodal_mtrssm_amd.fit import EarlyStopping, EpochMetrics, Trainer
from multimodal_mtrssm_amd.forecast import Forecast
from multimodal_mtrssm_amd.factory import make_mmtrssm, make_mrssm
from multimodal_mtrssm_amd.likelihood import LikelihoodBound, LikelihoodTable
from multimodal_mtrssm_amd.networks import MLP, MTRNN, Representation, Transition
from multimodal_mtrssm_amd.objective import likelihood
from multimodal_mtrssm_amd.optim import FlatAdamW, ReduceLROnPlateau, load_reference_checkpoint
from multimodal_mtrssm_amd.panel import EpisodePanel, EpisodePanelLogger, EpisodeVideo
from multimodal_mtrssm_amd.parallel import FlatDataParallel, GlobalRowNoise
from multimodal_mtrssm_amd.overshoot import LatentOvershoot, OvershootTable
from multimodal_mtrssm_amd.particle import ParticleFilter, ParticleTable
from multimodal_mtrssm_amd.probe import LatentProbe, LinearProbe, ProbeStats, ProbeTable
from multimodal_mtrssm_amd.schedule import ElboSchedule
from multimodal_mtrssm_amd.skill import ForecastSkill, SkillTable
from multimodal_mtrssm_amd.words import TransitionTable, WordTransitions
from multimodal_mtrssm_amd.state import MTState, State, cat_mtstates, cat_states, stack_mtstates, stack_states

__version__ = "0.1.0"

__all__ = [
    "MLP", "MTRNN", "Decoder", "DeviceEpisodeLoader", "DigitClassifier", "DigitStats", "DigitTrainer", "Distribution", "Encoder", "EpisodeBatch", "EpisodeDataModule", "ElboSchedule", "EpisodeDataModuleConfig", "EpisodePanel", "EpisodePanelLogger", "EpisodeVideo", "ExpertWeights", "FlatAdamW", "FlatDataParallel", "Forecast", "ForecastSkill", "GlobalRowNoise", "LatentProbe", "LikelihoodBound", "LikelihoodTable", "LinearProbe", "MTState", "MoPoE_MMTRSSM",
    "MoPoE_MRSSM", "ModalityDropout", "MultiOneHot", "MultiOneHotFactory", "ProbeStats", "ProbeTable", "ReduceLROnPlateau", "Representation", "SkillTable", "State", "StateCarry", "Transition", "TransitionTable", "WeightedMoPoE_MMTRSSM", "WeightedMoPoE_MRSSM", "WordTransitions", "cat_distribution",
    "cat_mtstates", "cat_states", "inject_uniforms", "kl_divergence", "likelihood", "load_reference_checkpoint", "make_mmtrssm", "make_mrssm",
    "stack_distribution", "stack_mtstates", "stack_states", "dropout_mask_reference", "tape_reference", "EarlyStopping", "EpochMetrics", "Trainer",
    "LatentOvershoot", "OvershootTable", "ParticleFilter", "ParticleTable", "CensusTable", "LatentCensus", "FrechetDistance", "FrechetTable",
    "CoherenceTable", "GenerationCoherence", "FeedAugment", "augment_key", "feed_augment_parameters", "feed_augment_reference",
]
