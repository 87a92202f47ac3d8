"""KL-in-reward on the GPU engine — drop-ins for verl's ``apply_kl_penalty`` and KL controllers
(called at agent_trainer.py:613-615 with ``algorithm.use_kl_in_reward``).

verl is an empty submodule in the reference: restated from verl's published ``ray_trainer`` /
``core_algos`` (the v0.3 line); parity is pinned to that restatement only
(tests/verl_restated_kl.py runs it on CPU torch as the checker).  The controllers are host
float math exactly as verl's; the tensor part — ``token_level_scores - beta * kld`` and the
per-row sums ``current_kl`` is made of — is one launch of ``rmi_kl_reward``.
"""
import numpy as np
import torch

from .. import distributed as rd
from ..ops import KL_KINDS
from ..protocol import DataProto
from . import core_algos
from .advantage import _warn_rank_local


class AdaptiveKLController:
    """verl AdaptiveKLController (https://arxiv.org/pdf/1909.08593.pdf)."""

    def __init__(self, init_kl_coef, target_kl, horizon):
        self.value = init_kl_coef
        self.target = target_kl
        self.horizon = horizon

    def update(self, current_kl, n_steps):
        proportional_error = np.clip(current_kl / self.target - 1, -0.2, 0.2)
        mult = 1 + proportional_error * n_steps / self.horizon
        self.value *= mult


class FixedKLController:
    """verl FixedKLController."""

    def __init__(self, kl_coef):
        self.value = kl_coef

    def update(self, current_kl, n_steps):
        pass


def get_kl_controller(kl_ctrl):
    """verl get_kl_controller over ``algorithm.kl_ctrl`` ({type, kl_coef[, target_kl, horizon]})."""
    if kl_ctrl.type == "fixed":
        return FixedKLController(kl_coef=kl_ctrl.kl_coef)
    if kl_ctrl.type == "adaptive":
        assert kl_ctrl.horizon > 0, f"horizon must be larger than 0. Got {kl_ctrl.horizon}"
        return AdaptiveKLController(init_kl_coef=kl_ctrl.kl_coef, target_kl=kl_ctrl.target_kl,
                                    horizon=kl_ctrl.horizon)
    raise NotImplementedError


def apply_kl_penalty(data: DataProto, kl_ctrl, kl_penalty="kl", multi_turn=False, process_group=None,
                     shard_rows=None):
    """verl apply_kl_penalty: sets ``token_level_rewards = token_level_scores - beta * kld``,
    updates ``kl_ctrl`` with the batch's ``current_kl`` and returns ``(data, metrics)``.  The
    mask is ``loss_mask[:, -L:]`` with ``multi_turn`` (as agent_trainer.py:614 passes), else
    ``attention_mask[:, -L:]``.  CPU tensors go to the device and the rewards come back.

    ``process_group``: the batch is this rank's shard; ``current_kl`` is the mean over the whole
    sharded batch's rows (every rank gathers the per-row sums in global row order and reduces them
    with the whole-batch kernel: the 1-GPU run's bits) and ``n_steps`` the global row count.
    ``shard_rows`` (every rank's row count) spares the gather its size exchange."""
    if kl_penalty not in KL_KINDS:  # "full" and unknown names, as verl's kl_penalty
        raise NotImplementedError
    _warn_rank_local("apply_kl_penalty current_kl", process_group)
    L = data.batch["responses"].size(1)
    scores = data.batch["token_level_scores"]
    mask = data.batch["loss_mask" if multi_turn else "attention_mask"][:, -L:]
    old, ref = data.batch["old_log_probs"], data.batch["ref_log_prob"]
    dev = core_algos._device(scores, old, ref, mask)
    beta = kl_ctrl.value
    rewards, row_stats = torch.ops.ragen_amd.kl_reward(
        core_algos._dev(scores.float(), dev), core_algos._dev(old.float(), dev), core_algos._dev(ref.float(), dev),
        core_algos._dev(mask, dev), float(beta), KL_KINDS[kl_penalty])
    if process_group is not None:
        row_stats = rd.gather_row_values(row_stats, process_group, shard_rows)
    n_steps = row_stats.shape[0]
    current_kl = torch.ops.ragen_amd.rows_mean(row_stats).item()
    kl_ctrl.update(current_kl=current_kl, n_steps=n_steps)
    data.batch["token_level_rewards"] = core_algos._back(scores.device, [rewards])[0]
    return data, {"actor/reward_kl_penalty": current_kl, "actor/reward_kl_penalty_coeff": beta}
