"""Event-timed rmi_kl_reward and rmi_grpo_outcome_scaled against their neighbours, one JSON line.

    python tools/kl_reward_time.py [--rounds 30] [--out profiles/kl_reward/line.json]

Per shape (8192 x 1093, the README's GAE shape, and 8192 x 4096, past the Infinity Cache), in
ONE process with the contenders interleaved round by round after a warm-up of every one of them:

  kl_reward        ops.kl_reward (kind kl), 17 B/token: three f32 and the mask in, rewards out
  gae              ops.gae (legacy, with row_stats) on the same shape: the same 17 B/token and a
                   serial recurrence kl_reward does not have
  eager            the torch composition of apply_kl_penalty's tensor part on the device
                   (kl_penalty, * mask, scores - beta * kld, masked_mean(axis=-1), mean)
  grpo / grpo_scaled  ops.grpo_outcome and ops.grpo_outcome_scaled (13 B/token + 4 B/row)

Times are device events around 10 back-to-back calls, per call (median and min over the rounds, in us); bytes/s is
the algorithm's traffic over the median.  No ratio is asserted: the line records them.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragen_amd import ops  # noqa: E402

SHAPES = ((8192, 1093), (8192, 4096))


def eager_kl(scores, old, ref, mask, beta):
    kld = (old - ref) * mask
    rewards = scores - beta * kld
    current = torch.mean((kld * mask).sum(-1) / mask.sum(-1), dim=0)
    return rewards, current


INNER = 10  # calls per event window (a window of one ~30 us call measures the events as much as the kernel)


def timed(fn, rounds_of):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(INNER):
        fn()
    e.record()
    e.synchronize()
    rounds_of.append(s.elapsed_time(e) * 1e3 / INNER)


def measure(B, L, rounds, dev):
    g = torch.Generator(device=dev).manual_seed(B + L)
    scores = torch.randn(B, L, device=dev, generator=g) * (torch.rand(B, L, device=dev, generator=g) < 0.2)
    old = -torch.rand(B, L, device=dev, generator=g) * 3
    ref = old + torch.randn(B, L, device=dev, generator=g) * 0.3
    lens = torch.randint(1, L + 1, (B, 1), device=dev, generator=g)
    mask = (torch.arange(L, device=dev)[None, :] >= L - lens).to(torch.uint8)
    values = torch.randn(B, L, device=dev, generator=g)
    stats3 = torch.empty(B, 3, dtype=torch.float64, device=dev)
    seg = torch.arange(B + 1, dtype=torch.int32, device=dev)
    rel = ops.length_weight_rows(mask)[1]
    fmask = mask.float()
    runs = {
        "kl_reward": lambda: ops.kl_reward(scores, old, ref, mask, 0.001, "kl"),
        "gae": lambda: ops.gae(scores, values, mask, 1.0, 1.0, "legacy", stats3),
        "eager": lambda: eager_kl(scores, old, ref, fmask, 0.001),
        "grpo": lambda: ops.grpo_outcome(scores, mask, seg, 1e-6, True),
        "grpo_scaled": lambda: ops.grpo_outcome_scaled(scores, mask, seg, 1e-6, True, rel),
    }
    for fn in runs.values():  # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            timed(fn, t[k])
    tok = B * L
    traffic = {"kl_reward": 17 * tok, "gae": 17 * tok, "grpo": 13 * tok, "grpo_scaled": 13 * tok + 4 * B}
    out = {"B": B, "L": L, "rounds": rounds}
    for k, v in t.items():
        med = statistics.median(v)
        out[k] = {"median_us": round(med, 2), "min_us": round(min(v), 2)}
        if k in traffic:
            out[k]["bytes"] = traffic[k]
            out[k]["TB_per_s"] = round(traffic[k] / med / 1e6, 3)
    out["kl_reward_over_gae"] = round(out["kl_reward"]["median_us"] / out["gae"]["median_us"], 3)
    out["eager_over_kl_reward"] = round(out["eager"]["median_us"] / out["kl_reward"]["median_us"], 3)
    out["grpo_scaled_over_grpo"] = round(out["grpo_scaled"]["median_us"] / out["grpo"]["median_us"], 3)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("kl_reward_time: needs the GPU (no fallback)")
    dev = torch.device("cuda", 0)
    line = json.dumps({"tool": "kl_reward_time", "device": torch.cuda.get_device_name(0),
                       "shapes": [measure(B, L, a.rounds, dev) for B, L in SHAPES]})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
