"""KL-in-reward (rmi_kl_reward / rmi_rows_mean, the apply_kl_penalty facade) and the GRPO
length weight (rmi_length_weight_*, rmi_grpo_outcome_scaled, rmi_row_div) on the GPU against the
CPU-torch restatement (tests/verl_restated_kl.py) and the reference-made fixture
tests/golden/length_weight.npz.  Rewards and advantages are compared bit for bit."""
import os
import uuid

import numpy as np
import pytest
import torch

import verl_restated_kl as vk
from ragen_amd.protocol import DataProto
from ragen_amd.trainer import (AdaptiveKLController, FixedKLController, apply_grpo_length_weight, apply_kl_penalty,
                               compute_advantage)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "length_weight.npz")
KINDS = {"kl": 0, "abs": 1, "mse": 2, "low_var_kl": 3}
SHAPES = [(1, 1), (3, 5), (7, 63), (5, 64), (6, 257), (33, 1093)]
BETAS = (0.0, 0.001, 0.7)
OPS = torch.ops.ragen_amd


def _inputs(B, L, seed=0, empty_row=True):
    """scores, old, ref f32[B, L] and a left-padded u8 mask with holes; row 0 fully masked out
    (empty_row) and row 1 fully on, where the batch has them."""
    rng = np.random.default_rng(seed + 1000 * B + L)
    scores = (rng.standard_normal((B, L)) * (rng.random((B, L)) < 0.2)).astype(np.float32)
    old = (-np.abs(rng.standard_normal((B, L))) * 2).astype(np.float32)
    ref = (old + rng.standard_normal((B, L)) * 0.3).astype(np.float32)
    lens = rng.integers(1, L + 1, B)
    m = (np.arange(L)[None, :] >= (L - lens)[:, None]).astype(np.uint8)
    m[rng.random((B, L)) < 0.05] = 0
    m[:, -1] = 1
    if B >= 2:
        m[1] = 1
        if empty_row:
            m[0] = 0
    return tuple(torch.from_numpy(x) for x in (scores, old, ref, m))


def _restated(scores, old, ref, m, beta, kind):
    kld = vk.kl_penalty(old, ref, kind) * m
    return (scores - beta * kld).numpy(), kld


def _shifted(x, device):
    """x on the device as the [1:] view of a buffer one element longer: contiguous, its base 4-B
    (the mask: 1-B) aligned but not 16-B (4-B) aligned."""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=device)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["kl", "abs", "mse"])
def test_kl_reward_rewards_bit_equal(device, kind, shape):
    s, o, r, m = _inputs(*shape)
    d = [x.to(device) for x in (s, o, r, m)]
    for beta in BETAS:
        want, _ = _restated(s, o, r, m, beta, kind)
        got, stats = OPS.kl_reward(*d, beta, KINDS[kind])
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        np.testing.assert_array_equal(stats[:, 1].cpu().numpy(), m.sum(1).double().numpy())
    # a bool mask arrives as a u8 view
    got, _ = OPS.kl_reward(d[0], d[1], d[2], d[3].bool(), 0.7, KINDS[kind])
    np.testing.assert_array_equal(got.cpu().numpy(), _restated(s, o, r, m, 0.7, kind)[0])


def test_kl_reward_streamed_launch(device):
    """The smallest batch whose traffic (17 B/token) passes 256 MiB: the launch that loads and
    stores nontemporally.  Same rewards bit for bit; its row sums equal those of the same rows
    launched in two halves (cached launches)."""
    B, L = 4100, 3857
    assert B * L * 17 > 256 * 1024 * 1024 and (B // 2 + 1) * L * 17 < 256 * 1024 * 1024
    g = torch.Generator().manual_seed(11)
    s = torch.randn(B, L, generator=g) * (torch.rand(B, L, generator=g) < 0.2)
    o = -torch.rand(B, L, generator=g) * 3
    r = o + torch.randn(B, L, generator=g) * 0.3
    m = (torch.arange(L)[None, :] >= torch.randint(0, L, (B, 1), generator=g)).to(torch.uint8)
    d = [x.to(device) for x in (s, o, r, m)]
    got, stats = OPS.kl_reward(*d, 0.7, 0)
    assert torch.equal(got.cpu(), s - 0.7 * ((o - r) * m))
    h = B // 2
    halves = torch.cat([OPS.kl_reward(*[x[a:b] for x in d], 0.7, 0)[1] for a, b in ((0, h), (h, B))])
    assert torch.equal(stats, halves)
    assert torch.equal(stats[:, 1].cpu(), m.sum(1).double())


@pytest.mark.parametrize("kind", ["kl", "abs", "mse", "low_var_kl"])
def test_kl_reward_unaligned_bases_take_the_scalar_path(device, kind):
    s, o, r, m = _inputs(7, 63)
    d = [_shifted(x, device) for x in (s, o, r, m)]
    aligned = OPS.kl_reward(*[x.to(device) for x in (s, o, r, m)], 0.7, KINDS[kind])
    got = OPS.kl_reward(*d, 0.7, KINDS[kind])
    if kind != "low_var_kl":
        np.testing.assert_array_equal(got[0].cpu().numpy(), _restated(s, o, r, m, 0.7, kind)[0])
    np.testing.assert_array_equal(got[0].cpu().numpy(), aligned[0].cpu().numpy())
    np.testing.assert_array_equal(got[1].cpu().numpy(), aligned[1].cpu().numpy())  # the row sums' bits too


@pytest.mark.parametrize("kind", ["kl", "abs", "mse"])
def test_kl_reward_non_finite_under_a_zero_mask_is_nan_as_in_torch(device, kind):
    s, o, r, m = _inputs(7, 63)
    off = np.flatnonzero(m[2].numpy() == 0)
    assert len(off) >= 3
    o[2, off[0]] = float("inf")
    r[2, off[1]] = float("nan")
    o[2, off[2]] = float("-inf")
    want, _ = _restated(s, o, r, m, 0.7, kind)
    assert np.isnan(want[2, off[:3]]).all() and np.isfinite(want[3:]).all()
    got, stats = OPS.kl_reward(*[x.to(device) for x in (s, o, r, m)], 0.7, KINDS[kind])
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert torch.isnan(stats[2, 0]) and torch.isfinite(stats[3:, 0]).all()


@pytest.mark.parametrize("shape", [(6, 257), (33, 1093)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["kl", "abs", "mse"])
def test_current_kl_within_the_fp64_bound(device, kind, shape):
    B, L = shape
    s, o, r, m = _inputs(B, L, empty_row=False)
    _, stats = OPS.kl_reward(*[x.to(device) for x in (s, o, r, m)], 0.001, KINDS[kind])
    np.testing.assert_array_equal(stats[:, 1].cpu().numpy(), m.sum(1).double().numpy())
    cur = OPS.rows_mean(stats).item()
    cur64, kmax = vk.current_kl_f64(o, r, m, kind)
    kld32 = vk.kl_penalty(o, r, kind) * m
    cur32 = torch.mean(vk.masked_mean(kld32, m, axis=-1), dim=0).item()
    bound = 2.0 ** -52 * (L + B) * kmax
    print(f"current_kl {kind} {B}x{L}: kernel {cur!r} f64 {cur64!r} f32 restatement {cur32!r} bound {bound:.3e} "
          f"|kernel-f64| {abs(cur - cur64):.3e} |f32-f64| {abs(cur32 - cur64):.3e}")
    assert abs(cur - cur64) <= bound
    assert abs(cur - cur64) <= abs(cur32 - cur64) + bound
    # the per-row quotient as its own vector gives the same bits
    per_row = (stats[:, 0] / stats[:, 1]).contiguous()
    assert OPS.rows_mean(per_row).item() == cur


def test_current_kl_is_nan_with_an_empty_row(device):
    s, o, r, m = _inputs(6, 257, empty_row=True)
    _, stats = OPS.kl_reward(*[x.to(device) for x in (s, o, r, m)], 0.001, 0)
    assert np.isnan(OPS.rows_mean(stats).item())
    kld = vk.kl_penalty(o, r, "kl") * m
    assert np.isnan(torch.mean(vk.masked_mean(kld, m, axis=-1), dim=0).item())  # as verl's masked_mean(axis=-1)


def test_low_var_kl_clamp_and_error(device):
    B, L = 33, 1093
    rng = np.random.default_rng(7)
    k = (rng.standard_normal((B, L)) * 3).astype(np.float32)
    old = (-np.abs(rng.standard_normal((B, L)))).astype(np.float32)
    special = np.array([-100, -12, 0, 3.3, 12, 100], np.float32)
    old[0, :6] = 0.0
    k[0, :6] = special
    ref = (old + k).astype(np.float32)
    old_t, ref_t = torch.from_numpy(old), torch.from_numpy(ref)
    kf = ref_t - old_t                       # the f32 k both sides start from
    np.testing.assert_array_equal(kf[0, :6].numpy(), special)
    k64 = kf.double()
    x64 = torch.exp(k64) - k64 - 1
    ones = torch.ones(B, L, dtype=torch.uint8)
    zeros = torch.zeros(B, L)
    cpu = vk.kl_penalty(old_t, ref_t, "low_var_kl")
    got, _ = OPS.kl_reward(zeros.to(device), old_t.to(device), ref_t.to(device), ones.to(device), 1.0, 3)
    dev = -got.cpu()                         # rewards = 0 - 1 * kld
    big = x64.abs() > 10
    assert big[0, [0, 1, 3, 4, 5]].all() and not big[0, 2]  # exp(3.3) - 4.3 = 22.8 is clamped too
    want_big = torch.where(x64[big] > 0, 10.0, -10.0).float()
    np.testing.assert_array_equal(dev[big].numpy(), want_big.numpy())
    np.testing.assert_array_equal(cpu[big].numpy(), want_big.numpy())
    assert dev[0, 2] == 0.0
    scale = torch.maximum(torch.maximum(torch.exp(k64), k64.abs()), torch.ones_like(k64)) * 2.0 ** -23
    e_dev = float(((dev.double() - x64).abs() / scale)[~big].max())
    e_cpu = float(((cpu.double() - x64).abs() / scale)[~big].max())
    print(f"low_var_kl error in units of max(exp k, |k|, 1) * 2^-23: kernel {e_dev:.4f} cpu f32 {e_cpu:.4f}")
    assert e_dev <= 2 * e_cpu


def _kl_batch(B, L, seed, where):
    s, o, r, m = _inputs(B, L, seed, empty_row=False)
    rng = np.random.default_rng(seed)
    loss_mask = torch.cat([torch.ones(B, 3, dtype=torch.bool), m.bool()], dim=1)   # wider than the responses
    am = torch.from_numpy((np.arange(L + 5)[None, :] >= rng.integers(0, L, B)[:, None]).astype(np.int64))
    t = {"responses": torch.zeros(B, L, dtype=torch.int64), "token_level_scores": s, "old_log_probs": o,
         "ref_log_prob": r, "loss_mask": loss_mask, "attention_mask": am}
    return {k: v.to(where) for k, v in t.items()}, t


@pytest.mark.parametrize("ctrl", ["fixed", "adaptive"])
@pytest.mark.parametrize("multi_turn", [True, False])
@pytest.mark.parametrize("where", ["cpu", "gpu"])
def test_apply_kl_penalty_facade(device, where, multi_turn, ctrl):
    B, L = 6, 257
    tensors, cpu = _kl_batch(B, L, 5, device if where == "gpu" else "cpu")
    make = (lambda mod: mod.FixedKLController(0.05)) if ctrl == "fixed" else \
        (lambda mod: mod.AdaptiveKLController(0.05, 0.01, 100))
    import ragen_amd.trainer.kl as kl_mod
    ours, ref = make(kl_mod), make(vk)
    assert isinstance(ours, (FixedKLController, AdaptiveKLController))
    data = DataProto.from_dict(tensors)
    out, metrics = apply_kl_penalty(data, ours, "abs", multi_turn=multi_turn)
    want, rmetrics = vk.apply_kl_penalty(cpu, ref, "abs", multi_turn=multi_turn)
    rew = out.batch["token_level_rewards"]
    assert out is data and rew.device.type == ("cuda" if where == "gpu" else "cpu")
    np.testing.assert_array_equal(rew.cpu().numpy(), want.numpy())
    assert list(metrics) == ["actor/reward_kl_penalty", "actor/reward_kl_penalty_coeff"]
    assert metrics["actor/reward_kl_penalty_coeff"] == rmetrics["actor/reward_kl_penalty_coeff"] == 0.05
    mask = (cpu["loss_mask"] if multi_turn else cpu["attention_mask"])[:, -L:]
    cur64, kmax = vk.current_kl_f64(cpu["old_log_probs"], cpu["ref_log_prob"], mask, "abs")
    cur = metrics["actor/reward_kl_penalty"]
    assert isinstance(cur, float) and abs(cur - cur64) <= 2.0 ** -52 * (L + B) * kmax
    # the restatement sums in f32: (L + B) roundings of 2^-24 relative to max |kld|
    assert abs(cur - rmetrics["actor/reward_kl_penalty"]) <= 2.0 ** -23 * (L + B) * kmax
    # the controller: exactly the restated update fed the engine's current_kl (n_steps = batch size)
    fed = make(vk)
    fed.update(current_kl=cur, n_steps=B)
    assert ours.value == fed.value
    assert ours.value == pytest.approx(ref.value, rel=1e-5)
    if ctrl == "adaptive":
        assert ours.value != 0.05


def test_apply_kl_penalty_full_raises(device):
    tensors, _ = _kl_batch(3, 5, 1, device)
    for name in ("full", "nonsense"):
        with pytest.raises(NotImplementedError):
            apply_kl_penalty(DataProto.from_dict(tensors), FixedKLController(0.1), name)
        with pytest.raises(NotImplementedError):
            vk.kl_penalty(tensors["old_log_probs"].cpu(), tensors["ref_log_prob"].cpu(), name)


@pytest.mark.parametrize("split", [16, 15], ids=["16+17", "15+18"])
def test_shards_equal_the_whole_batch(device, split):
    """Row shards (16 + 17, and 15 + 18 whose second shard starts at a base that is not 16-B
    aligned) reduce to the whole batch's bits: the per-row sums, current_kl and the length
    weight's rel vector."""
    B, L = 33, 1093
    s, o, r, m = [x.to(device) for x in _inputs(B, L, empty_row=False)]
    _, whole = OPS.kl_reward(s, o, r, m, 0.001, 0)
    parts = [OPS.kl_reward(s[a:b], o[a:b], r[a:b], m[a:b], 0.001, 0) for a, b in ((0, split), (split, B))]
    stats = torch.cat([p[1] for p in parts])
    np.testing.assert_array_equal(stats.cpu().numpy(), whole.cpu().numpy())
    assert OPS.rows_mean(stats).item() == OPS.rows_mean(whole).item()
    count, rel = OPS.length_weight_rows(m)
    counts = torch.cat([OPS.length_weight_rows(m[a:b])[0] for a, b in ((0, split), (split, B))])
    np.testing.assert_array_equal(counts.cpu().numpy(), m.sum(1).cpu().numpy())
    np.testing.assert_array_equal(counts.cpu().numpy(), count.cpu().numpy())
    np.testing.assert_array_equal(OPS.length_weight_finalize(counts).cpu().numpy(), rel.cpu().numpy())


# ------------------------------------------------------------------ the length weight
def _golden():
    return {k: torch.from_numpy(v) for k, v in np.load(GOLDEN).items()}


def _grpo_data(rewards, mask, uid, where):
    return DataProto.from_dict({"token_level_rewards": rewards.to(where), "response_mask": mask.to(where)},
                               {"uid": np.array(uid, dtype=object)})


@pytest.mark.parametrize("where", ["cpu", "gpu"])
def test_length_weight_equals_the_fixture(device, where):
    g = _golden()
    where = device if where == "gpu" else "cpu"
    uid = [str(uuid.uuid4()) for _ in range(40)]
    fused = compute_advantage(_grpo_data(g["token_level_rewards"], g["response_mask"], uid, where), "grpo",
                              grpo_advantage_length_weight=True)
    assert fused.batch["advantages"].device.type == torch.device(where).type
    np.testing.assert_array_equal(fused.batch["advantages"].cpu().numpy(), g["grpo_weighted"].numpy())
    np.testing.assert_array_equal(fused.batch["returns"].cpu().numpy(), g["grpo_advantages"].numpy())  # unweighted
    plain = compute_advantage(_grpo_data(g["token_level_rewards"], g["response_mask"], uid, where), "grpo")
    np.testing.assert_array_equal(plain.batch["advantages"].cpu().numpy(), g["grpo_advantages"].numpy())
    after = apply_grpo_length_weight(plain)
    assert after is plain
    np.testing.assert_array_equal(after.batch["advantages"].cpu().numpy(), g["grpo_weighted"].numpy())
    np.testing.assert_array_equal(after.batch["returns"].cpu().numpy(), g["grpo_advantages"].numpy())
    # an arbitrary advantage tensor (the fixture's random one) through the standalone step
    free = DataProto.from_dict({"advantages": g["advantages"].to(where), "response_mask": g["response_mask"].to(where)})
    np.testing.assert_array_equal(apply_grpo_length_weight(free).batch["advantages"].cpu().numpy(),
                                  g["weighted"].numpy())
    # other estimators ignore the key, as agent_trainer.py:636 does
    d = _grpo_data(g["token_level_rewards"], g["response_mask"], uid, where)
    a = compute_advantage(d, "rloo", grpo_advantage_length_weight=True).batch["advantages"].cpu().numpy()
    b = compute_advantage(_grpo_data(g["token_level_rewards"], g["response_mask"], uid, where),
                          "rloo").batch["advantages"].cpu().numpy()
    np.testing.assert_array_equal(a, b)


def _uneven(B=96, L=57, seed=0, groups=12):  # as test_verl_estimators._batch
    rng = np.random.default_rng(seed)
    r = (rng.standard_normal((B, L)) * (rng.random((B, L)) < 0.2)).astype(np.float32)
    lens = rng.integers(1, L + 1, B)
    m = (np.arange(L)[None, :] >= (L - lens)[:, None]).astype(np.uint8)
    m[rng.random((B, L)) < 0.05] = 0
    m[:, -1] = 1
    uid = [f"u{int(g)}" for g in rng.integers(0, groups, B)]
    uid[0] = "solo"
    return torch.from_numpy(r), torch.from_numpy(m), uid


@pytest.mark.parametrize("case", ["uneven_96x57", "one_group_of_70", "all_zero_mask"])
@pytest.mark.parametrize("norm_by_std", [True, False])
def test_length_weight_fused_equals_the_reference_order(device, case, norm_by_std):
    """compute_advantage with the weight fused == the unweighted device advantages put through
    the reference's lines on the CPU: shuffled uneven groups, a group past the 64 register-kept
    row scores, and an all-zero mask (rel = inf: the advantages are 0)."""
    if case == "uneven_96x57":
        r, m, uid = _uneven()
    elif case == "one_group_of_70":
        r, m, _ = _uneven(70, 57, seed=3)
        uid = ["g"] * 70
    else:
        r, m, uid = _uneven(8, 57, seed=4)
        m = torch.zeros_like(m)
    kw = dict(norm_adv_by_std_in_grpo=norm_by_std)
    plain = compute_advantage(_grpo_data(r, m, uid, device), "grpo", **kw).batch["advantages"].cpu()
    want = vk.grpo_length_weight(plain, m.to(torch.int64))
    if case == "all_zero_mask":
        assert not want.any() and not torch.isnan(want).any()
    else:
        assert (want != plain).any()
    fused = compute_advantage(_grpo_data(r, m, uid, device), "grpo", grpo_advantage_length_weight=True, **kw)
    np.testing.assert_array_equal(fused.batch["advantages"].cpu().numpy(), want.numpy())
    np.testing.assert_array_equal(fused.batch["returns"].cpu().numpy(), plain.numpy())
    after = apply_grpo_length_weight(compute_advantage(_grpo_data(r, m, uid, device), "grpo", **kw))
    np.testing.assert_array_equal(after.batch["advantages"].cpu().numpy(), want.numpy())


def test_grpo_outcome_scaled_without_a_scale_is_grpo_outcome(device):
    r, m, uid = _uneven()
    seg = torch.tensor([0, 10, 11, 50, 96], dtype=torch.int32, device=device)
    a = OPS.grpo_outcome(r.to(device), m.to(device), seg, 1e-6, True)
    b = OPS.grpo_outcome_scaled(r.to(device), m.to(device), seg, 1e-6, True, None)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
    # an unaligned advantage tensor takes row_div's scalar path
    adv = a[0].clone()
    rel = OPS.length_weight_rows(m.to(device))[1]
    sh = _shifted(adv.cpu(), device)
    OPS.row_div_(adv, rel)
    OPS.row_div_(sh, rel)
    np.testing.assert_array_equal(sh.cpu().numpy(), adv.cpu().numpy())
    np.testing.assert_array_equal(adv.cpu().numpy(), vk.grpo_length_weight(a[0].cpu(), m.to(torch.int64)).numpy())


def test_process_group_path_equals_the_local_one(device):
    """With a (1-rank, gloo) process group the facades gather the per-row values and reduce them
    with the whole-batch kernels: the same rewards, metrics, controller value and advantages as
    without a group."""
    import socket
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        B, L = 6, 257
        tensors, _ = _kl_batch(B, L, 9, device)
        a, b = AdaptiveKLController(0.05, 0.01, 100), AdaptiveKLController(0.05, 0.01, 100)
        local, lm = apply_kl_penalty(DataProto.from_dict(dict(tensors)), a, "mse", multi_turn=True)
        grp, gm = apply_kl_penalty(DataProto.from_dict(dict(tensors)), b, "mse", multi_turn=True,
                                   process_group=dist.group.WORLD, shard_rows=[B])
        assert lm == gm and a.value == b.value
        assert torch.equal(local.batch["token_level_rewards"], grp.batch["token_level_rewards"])
        r, m, uid = _uneven()
        kw = dict(grpo_advantage_length_weight=True)
        want = compute_advantage(_grpo_data(r, m, uid, device), "grpo", **kw).batch["advantages"]
        got = compute_advantage(_grpo_data(r, m, uid, device), "grpo", process_group=dist.group.WORLD,
                                shard_rows=[r.shape[0]], **kw).batch["advantages"]
        assert torch.equal(want, got)
        d = compute_advantage(_grpo_data(r, m, uid, device), "grpo")
        assert torch.equal(apply_grpo_length_weight(d, process_group=dist.group.WORLD).batch["advantages"], want)
    finally:
        dist.destroy_process_group()
