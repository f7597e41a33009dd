"""vqhmm — MI355X-native (gfx950) implementation of the VAE_HMM training hot path
of yashnaray/VQ-VAE-HMM-model.

Drop-in surface (VQ_VAE_HMM_fixed.py): VAE_HMM, Encoder, Prior, Decoder,
train_model, RandomChunkDataset, collate_fn — plus the hard-regime kernels
vq_argmin / forward_backward / viterbi.  All compute runs in hand-written HIP
kernels in libvqhmm.so; there is no CPU fallback.
"""
import os as _os

# Kernel arguments in device memory instead of host memory: a dispatch's argument fetch then does not cross
# PCIe, which is most of a short launch's fixed cost here (tools/gpu_kernarg_ab.sh, alternating on one box:
# B = 128 step 0.1082 -> 0.0939 ms, its DP form 0.1149 -> 0.0995, cfg2 0.4342 -> 0.4199).  Read when the HIP
# runtime initialises, i.e. effective when this package is imported before the process's first GPU call.
_os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

from . import _ext  # noqa: E402,F401
from .backtest import Backtest, backtest  # noqa: E402,F401
from .checkpoint import load_checkpoint, load_encoder, save_checkpoint, save_encoder  # noqa: E402,F401
from .codebook import Codebook  # noqa: E402,F401
from .codehmm import CodeHMM, code_log_prob  # noqa: E402,F401
from .codehmm_ensemble import CodeHMMEnsemble  # noqa: E402,F401
from .gauss_hmm import (GaussianHMM, Scenarios, gauss_full_log_prob, gauss_log_prob,  # noqa: E402,F401
                        regime_covariance, regime_moments, scenario_summary)
from .gauss_hmm_ensemble import GaussianHMMEnsemble  # noqa: E402,F401
from .data import DeviceChunkLoader, RandomChunkDataset, collate_fn  # noqa: E402,F401
from .hmm import (forward_backward, forward_filter, pairwise_posteriors, quantize, regime_argmax,  # noqa: E402,F401
                  sample_posterior_paths, simulate_paths, viterbi, vq_argmin)
from .infer import (filtered_regimes, hard_regimes, infer, prior_viterbi, sampled_regimes,  # noqa: E402,F401
                    simulate_regimes, viterbi_regimes)
from .model import PARAM_ORDER, VAE_HMM, Decoder, Encoder, Prior  # noqa: E402,F401
from .train import Trainer, TrainState, train_model  # noqa: E402,F401

__all__ = ["VAE_HMM", "Encoder", "Prior", "Decoder", "train_model", "Trainer", "TrainState", "RandomChunkDataset",
           "collate_fn", "DeviceChunkLoader", "vq_argmin", "quantize", "regime_argmax", "viterbi", "forward_backward", "PARAM_ORDER",
           "save_checkpoint", "load_checkpoint", "save_encoder", "load_encoder", "infer", "hard_regimes", "viterbi_regimes",
           "prior_viterbi", "forward_filter", "pairwise_posteriors", "filtered_regimes", "CodeHMM", "CodeHMMEnsemble", "code_log_prob", "Codebook", "GaussianHMM", "gauss_log_prob",
           "gauss_full_log_prob", "regime_moments", "regime_covariance", "GaussianHMMEnsemble", "Scenarios", "scenario_summary",
           "sample_posterior_paths", "simulate_paths", "sampled_regimes", "simulate_regimes", "backtest", "Backtest"]
