"""pcdet.query_strategies factory (pcdet/query_strategies/__init__.py:12-29): the reference's eight strategies plus the
unregistered `bald`. `llal` needs the loss-prediction module of the LLAL detector variant (ROI_HEAD.LOSS_NET,
pcdet.model_cfgs.pv_rcnn_llal_cfg)."""
from .badge_sampling import BadgeSampling
from .bald_sampling import BALDSampling
from .confidence_sampling import ConfidenceSampling
from .coreset_sampling import CoresetSampling
from .crb_sampling import CRBSampling
from .entropy_sampling import EntropySampling
from .llal_sampling import LLALSampling
from .montecarlo_sampling import MonteCarloSampling
from .random_sampling import RandomSampling
from .strategy import Strategy  # noqa: F401

__factory = {
    'random': RandomSampling,
    'entropy': EntropySampling,
    'confidence': ConfidenceSampling,
    'bald': BALDSampling,
    'montecarlo': MonteCarloSampling,
    'coreset': CoresetSampling,
    'badge': BadgeSampling,
    'crb': CRBSampling,
    'llal': LLALSampling,
}


def names():
    return sorted(__factory.keys())


def build_strategy(method, model, labelled_loader, unlabelled_loader, rank, active_label_dir, cfg):
    if method not in __factory:
        raise KeyError('Unknown query strategy: {} (available: {})'.format(method, names()))
    return __factory[method](model, labelled_loader, unlabelled_loader, rank, active_label_dir, cfg)
