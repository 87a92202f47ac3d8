"""verl's KL-in-reward step as published in verl.trainer.ppo (ray_trainer.apply_kl_penalty,
core_algos.kl_penalty and the KL controllers; the v0.3 line — verl is an empty submodule in the
reference, agent_trainer.py:613-615 calls these), restated on CPU torch, and the reference's own
length weight (agent_trainer.py:636-641) restated next to it.  Test infrastructure only: the
checker for the device kernels, run with the reference's own numerics (torch CPU f32 ops).
Parity beyond this restatement is unpinned for the KL step: no reference vectors exist for it;
the length weight is pinned by tests/golden/length_weight.npz, which the reference's own lines
produced."""
import numpy as np
import torch


def masked_mean(values, mask, axis=None):  # as tests/golden/refshim.py:249 (no epsilon)
    return (values * mask).sum(axis=axis) / mask.sum(axis=axis)


def kl_penalty(logprob, ref_logprob, kl_penalty):
    if kl_penalty == "kl":
        return logprob - ref_logprob
    if kl_penalty == "abs":
        return (logprob - ref_logprob).abs()
    if kl_penalty == "mse":
        return 0.5 * (logprob - ref_logprob).square()
    if kl_penalty == "low_var_kl":
        kl = ref_logprob - logprob
        ratio = torch.exp(kl)
        kld = (ratio - kl - 1).contiguous()
        return torch.clamp(kld, min=-10, max=10)
    if kl_penalty == "full":
        raise NotImplementedError
    raise NotImplementedError


class AdaptiveKLController:
    def __init__(self, init_kl_coef, target_kl, horizon):
        self.value = init_kl_coef
        self.target = target_kl
        self.horizon = horizon

    def update(self, current_kl, n_steps):
        target = self.target
        proportional_error = np.clip(current_kl / target - 1, -0.2, 0.2)
        mult = 1 + proportional_error * n_steps / self.horizon
        self.value *= mult


class FixedKLController:
    def __init__(self, kl_coef):
        self.value = kl_coef

    def update(self, current_kl, n_steps):
        pass


def apply_kl_penalty(batch, kl_ctrl, kl_penalty_name="kl", multi_turn=False):
    """batch: a dict of CPU tensors.  -> (token_level_rewards, metrics); updates kl_ctrl."""
    response_length = batch["responses"].size(1)
    token_level_scores = batch["token_level_scores"]
    batch_size = token_level_scores.shape[0]
    if multi_turn:
        response_mask = batch["loss_mask"][:, -response_length:]
    else:
        response_mask = batch["attention_mask"][:, -response_length:]
    kld = kl_penalty(batch["old_log_probs"], batch["ref_log_prob"], kl_penalty=kl_penalty_name)
    kld = kld * response_mask
    beta = kl_ctrl.value
    token_level_rewards = token_level_scores - beta * kld
    current_kl = masked_mean(kld, mask=response_mask, axis=-1)
    current_kl = torch.mean(current_kl, dim=0).item()
    kl_ctrl.update(current_kl=current_kl, n_steps=batch_size)
    metrics = {"actor/reward_kl_penalty": current_kl, "actor/reward_kl_penalty_coeff": beta}
    return token_level_rewards, metrics


def current_kl_f64(old_log_probs, ref_log_prob, response_mask, kl_penalty_name="kl"):
    """current_kl of the f32 kld values with every reduction in float64 -> (value, max |kld|)."""
    kld = kl_penalty(old_log_probs, ref_log_prob, kl_penalty_name) * response_mask
    k64, m64 = kld.double(), response_mask.double()
    cur = torch.mean((k64 * m64).sum(-1) / m64.sum(-1), dim=0).item()
    fin = kld[torch.isfinite(kld)]
    return cur, (float(fin.abs().max()) if fin.numel() else 0.0)


def grpo_length_weight(advantages, response_mask):
    """agent_trainer.py:637-641 restated."""
    response_relative_lengths = (torch.sum(response_mask, dim=-1) + 1e-6) / torch.sum(response_mask, dim=-1).float().mean()
    return advantages / response_relative_lengths.unsqueeze(-1)
