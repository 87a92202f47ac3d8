"""The adv block of RayAgentTrainer.fit with use_kl_in_reward and grpo_advantage_length_weight
(agent_trainer.py:612-641) on a SimpleSokoban 8 x 16 rollout with stub log-prob workers:
apply_kl_penalty(multi_turn=True) with the adaptive controller -> compute_advantage("grpo") ->
the length weight, against the CPU-torch restatement of those lines.  Rewards and advantages
are compared bit for bit, the metrics within the fp64 bound of tests/test_gpu_kl_reward.py.

The restated GRPO forms each row's score as rmi_grpo_outcome documents it (include/ragen_amd.h,
advantage.hip: the row is summed in fp64 and rounded to f32 once), which is what makes a
bit-for-bit comparison of the advantages meaningful: torch's f32 `.sum(dim=-1)` of a row of
several hundred KL-penalised rewards rounds at every partial sum, in an order the engine does
not reproduce (it is compared too, to 1e-6 as tests/test_gpu_fit.py does).  Everything else —
the KL step, groups of one under unique uids, the broadcast over the loss mask and the length
weight over the response mask — is verl's / the reference's f32 arithmetic in its order."""
import uuid

import numpy as np
import pytest
import torch

import verl_restated_kl as vk
from test_gpu_fit import _rollout
from ragen_amd.protocol import DataProto
from ragen_amd.trainer import (AdaptiveKLController, DummyRewardManager, apply_grpo_length_weight, apply_kl_penalty,
                               compute_advantage, compute_reward)

pytestmark = pytest.mark.gpu


class StubLogProbWorkers:
    """actor_rollout_wg.compute_log_prob / ref_policy_wg.compute_ref_log_prob as DP workers."""

    def __init__(self, world=4):
        self.world = world

    def _dp(self, data, fn):
        return DataProto.concat([fn(p) for p in data.chunk(self.world)])

    def compute_log_prob(self, data):
        return self._dp(data, lambda p: DataProto.from_dict(
            {"old_log_probs": -(p.batch["responses"].float() % 7) / 10}))

    def compute_ref_log_prob(self, data):
        return self._dp(data, lambda p: DataProto.from_dict(
            {"ref_log_prob": -(p.batch["responses"].float() % 11) / 13 - 0.01}))


def _restated_grpo_unique_uids(token_level_rewards, mask, epsilon=1e-6, f32_sum=False):
    """verl compute_grpo_outcome_advantage with every uid unique (agent_trainer.py:551-552):
    id2mean = 0, id2std = 1.  The row score: see the module docstring."""
    scores = token_level_rewards.sum(dim=-1) if f32_sum else token_level_rewards.double().sum(dim=-1).float()
    scores = (scores - torch.tensor(0.0)) / (torch.tensor(1.0) + epsilon)
    return scores.unsqueeze(-1) * mask


def test_fit_kl_grpo_length_weight_sequence(device):
    groups, gs = 8, 16
    batch, tok = _rollout(device, groups, gs)
    B = len(batch)
    batch.non_tensor_batch["uid"] = np.array([str(uuid.uuid4()) for _ in range(B)], dtype=object)
    batch.batch["response_mask"] = batch.batch["loss_mask"]
    reward_tensor, _ = compute_reward(batch, DummyRewardManager(tok, 0))
    wg = StubLogProbWorkers()
    batch = batch.union(wg.compute_log_prob(batch)).union(wg.compute_ref_log_prob(batch))
    batch.batch["token_level_scores"] = reward_tensor
    cpu = {k: v.clone() for k, v in batch.batch.items()}
    L = cpu["responses"].size(1)

    # :612-615
    ctrl, rctrl = AdaptiveKLController(0.001, 0.01, 100), vk.AdaptiveKLController(0.001, 0.01, 100)
    batch, kl_metrics = apply_kl_penalty(batch, kl_ctrl=ctrl, kl_penalty="kl", multi_turn=True)
    want_rewards, rmetrics = vk.apply_kl_penalty(cpu, rctrl, "kl", multi_turn=True)
    rewards = batch.batch["token_level_rewards"]
    assert rewards.device.type == "cpu"
    np.testing.assert_array_equal(rewards.numpy(), want_rewards.numpy())
    assert (rewards != cpu["token_level_scores"]).any()
    mask = cpu["loss_mask"][:, -L:]
    cur64, kmax = vk.current_kl_f64(cpu["old_log_probs"], cpu["ref_log_prob"], mask, "kl")
    cur = kl_metrics["actor/reward_kl_penalty"]
    bound = 2.0 ** -52 * (L + B) * kmax
    print(f"fit current_kl: engine {cur!r} f64 {cur64!r} f32 restatement {rmetrics['actor/reward_kl_penalty']!r} "
          f"bound {bound:.3e}")
    assert abs(cur - cur64) <= bound
    assert abs(cur - cur64) <= abs(rmetrics["actor/reward_kl_penalty"] - cur64) + bound
    assert kl_metrics["actor/reward_kl_penalty_coeff"] == rmetrics["actor/reward_kl_penalty_coeff"] == 0.001
    fed = vk.AdaptiveKLController(0.001, 0.01, 100)
    fed.update(current_kl=cur, n_steps=B)
    assert ctrl.value == fed.value and ctrl.value == pytest.approx(rctrl.value, rel=1e-6)

    # :623-633, then :636-641
    kw = dict(gamma=1.0, lam=1.0, num_repeat=1, norm_adv_by_std_in_grpo=True, multi_turn=True, high_level_gamma=0.95,
              bi_level_gae=False)
    want_adv = _restated_grpo_unique_uids(want_rewards, mask)
    want_weighted = vk.grpo_length_weight(want_adv, cpu["response_mask"])
    plain = compute_advantage(DataProto(batch.batch.clone(), dict(batch.non_tensor_batch)), "grpo", **kw)
    np.testing.assert_array_equal(plain.batch["advantages"].numpy(), want_adv.numpy())
    np.testing.assert_allclose(plain.batch["advantages"].numpy(),
                               _restated_grpo_unique_uids(want_rewards, mask, f32_sum=True).numpy(), rtol=1e-6, atol=1e-6)
    after = apply_grpo_length_weight(plain)
    np.testing.assert_array_equal(after.batch["advantages"].numpy(), want_weighted.numpy())
    assert (want_weighted != want_adv).any()
    fused = compute_advantage(batch, "grpo", grpo_advantage_length_weight=True, **kw)
    assert fused.batch["advantages"].device.type == "cpu"
    np.testing.assert_array_equal(fused.batch["advantages"].numpy(), want_weighted.numpy())
    np.testing.assert_array_equal(fused.batch["returns"].numpy(), want_adv.numpy())
