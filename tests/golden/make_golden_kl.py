"""Generate tests/golden/length_weight.npz by RUNNING THE READ-ONLY REFERENCE's own
grpo_advantage_length_weight lines (ragen/trainer/agent_trainer.py:637-641).

TEST INFRASTRUCTURE, run where the reference tree exists:

    python tests/golden/make_golden_kl.py <path to the reference tree>

The five statements are read from the reference's file at generation time, dedented and
executed on a stub batch; only data (the inputs, the mask, the weighted output) is written, no
reference source is stored.  Inputs: random advantages at (B, L) = (40, 64) whose rows carry
the mask counts {0, 1, 2, 15, 16, 17, 31, 32, 33, 64} (four times over): the counts around 16
and 32 pin the f32 rounding of `sum + 1e-6` (16 -> 16.000001907, 32 -> 32.0).  A second input
has the shape GRPO itself produces (one score per row, broadcast over the mask): random
token-level rewards and their GRPO advantages under unique uids (verl
compute_grpo_outcome_advantage with groups of one: (sum_t r - 0) / (1 + 1e-6), times the mask),
so compute_advantage can be driven to the same weighted array.
"""
import os
import sys
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
COUNTS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 64)
B, L = 40, 64


def reference_lines(ref_root):
    path = os.path.join(ref_root, "ragen", "trainer", "agent_trainer.py")
    lines = open(path).read().split("\n")[636:641]  # file lines 637-641
    src = textwrap.dedent("\n".join(lines))
    assert "response_relative_lengths" in src and src.lstrip().startswith("response_mask = batch.batch"), src
    return src


def weigh(src, mask, adv):
    batch = types.SimpleNamespace(batch={"response_mask": torch.from_numpy(mask.astype(np.int64)),
                                         "advantages": torch.from_numpy(adv.copy())})
    exec(compile(src, "agent_trainer.py:637-641", "exec"), {"torch": torch, "batch": batch})
    out = batch.batch["advantages"].numpy()
    assert out.dtype == np.float32 and out.shape == adv.shape
    return out


def main(ref_root):
    rng = np.random.default_rng(20)
    adv = rng.standard_normal((B, L)).astype(np.float32)
    mask = np.zeros((B, L), np.uint8)
    for b in range(B):
        n = COUNTS[b % len(COUNTS)]
        cols = np.arange(L - n, L) if b < 20 else rng.permutation(L)[:n]  # left-padded rows, then holes
        mask[b, cols] = 1
    adv *= mask  # GRPO advantages are zero outside the mask
    adv[3, :] = -adv[3, :].__abs__()  # a row of negative advantages (the sign of its zeros)
    src = reference_lines(ref_root)
    out = weigh(src, mask, adv)
    # the GRPO-shaped input: one reward per row on its last column, groups of one
    rewards = np.zeros((B, L), np.float32)
    rewards[:, -1] = rng.standard_normal(B).astype(np.float32) * 3
    scores = torch.from_numpy(rewards).sum(dim=-1)
    scores = (scores - torch.tensor(0.0)) / (torch.tensor(1.0) + 1e-6)
    grpo_adv = (scores.unsqueeze(-1) * torch.from_numpy(mask)).numpy()
    grpo_out = weigh(src, mask, grpo_adv)
    np.savez_compressed(os.path.join(HERE, "length_weight.npz"), advantages=adv, response_mask=mask, weighted=out,
                        token_level_rewards=rewards, grpo_advantages=grpo_adv, grpo_weighted=grpo_out)
    print("length_weight.npz", out.shape, "rows weighted:", int((out != adv).any(1).sum()))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["RAGEN_REFERENCE"])
