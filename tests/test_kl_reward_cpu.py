"""KL-in-reward and the GRPO length weight, the parts that need no GPU: the KL controllers
against the verl restatement, the new C entry points' argument checks (they return before any
HIP call, like the formulate chain's), the length-weight fixture against its restatement, the
config keys, and the gather helper over a gloo world of 2."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import verl_restated_kl as vk
from ragen_amd import _lib
from ragen_amd import distributed as rd
from ragen_amd.config import AttrDict, default_config
from ragen_amd.trainer import AdaptiveKLController, FixedKLController, get_kl_controller

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "length_weight.npz")


def test_controllers_equal_the_restatement_over_50_updates():
    rng = np.random.default_rng(3)
    kls = rng.normal(0.01, 0.004, 50)
    kls[5], kls[6] = 1.0, -1.0           # far above / below the target: the clip at +-0.2
    kls[20], kls[21] = 0.01 * 1.2, 0.01 * 0.8  # at the clip's edges
    ours, ref = AdaptiveKLController(0.001, 0.01, 100), vk.AdaptiveKLController(0.001, 0.01, 100)
    fixed, rfixed = FixedKLController(0.05), vk.FixedKLController(0.05)
    for i, kl in enumerate(kls):
        before = ours.value
        ours.update(current_kl=float(kl), n_steps=8 + i)
        ref.update(current_kl=float(kl), n_steps=8 + i)
        fixed.update(current_kl=float(kl), n_steps=8 + i)
        rfixed.update(current_kl=float(kl), n_steps=8 + i)
        assert ours.value == ref.value and fixed.value == rfixed.value == 0.05
        if i == 5:
            assert ours.value == before * (1 + 0.2 * (8 + i) / 100)
        if i == 6:
            assert ours.value == before * (1 + -0.2 * (8 + i) / 100)
    ours.update(current_kl=float("nan"), n_steps=8)
    ref.update(current_kl=float("nan"), n_steps=8)
    assert math.isnan(ours.value) and math.isnan(ref.value)


def test_get_kl_controller():
    c = get_kl_controller(AttrDict(type="fixed", kl_coef=0.001))
    assert isinstance(c, FixedKLController) and c.value == 0.001
    c = get_kl_controller(AttrDict(type="adaptive", kl_coef=0.002, target_kl=0.01, horizon=100))
    assert isinstance(c, AdaptiveKLController) and (c.value, c.target, c.horizon) == (0.002, 0.01, 100)
    with pytest.raises(AssertionError):
        get_kl_controller(AttrDict(type="adaptive", kl_coef=0.002, target_kl=0.01, horizon=0))
    with pytest.raises(NotImplementedError):
        get_kl_controller(AttrDict(type="pid", kl_coef=0.002))
    c = get_kl_controller(default_config().algorithm.kl_ctrl)
    assert isinstance(c, FixedKLController) and c.value == 0.0


def test_entry_points_check_arguments_before_any_hip_call():
    L = _lib.lib()
    p = 64  # a non-null address that is never dereferenced: every call below returns before a launch
    E, OK = _lib.RMI_EINVAL, _lib.RMI_OK
    kl = lambda **k: L.rmi_kl_reward(*[k.get(n, d) for n, d in (
        ("scores", p), ("old", p), ("ref", p), ("mask", p), ("B", 4), ("L", 8), ("beta", 0.1), ("kind", 0),
        ("rewards", p), ("row_stats", p), ("stream", None))])
    for name in ("scores", "old", "ref", "mask", "rewards", "row_stats"):
        assert kl(**{name: None}) == E, name
    assert kl(B=-1) == E and kl(L=-1) == E and kl(kind=-1) == E and kl(kind=4) == E
    assert kl(B=0) == OK and kl(L=0) == OK and kl(B=0, kind=3) == OK
    assert L.rmi_rows_mean(None, None, 4, 1, p, None) == E
    assert L.rmi_rows_mean(p, None, 4, 1, None, None) == E
    assert L.rmi_rows_mean(p, None, -1, 1, p, None) == E
    assert L.rmi_rows_mean(p, None, 4, 0, p, None) == E
    assert L.rmi_rows_mean(p, p, 0, 2, p, None) == OK
    assert L.rmi_length_weight_rows(None, 4, 8, p, p, None) == E
    assert L.rmi_length_weight_rows(p, 4, 8, None, p, None) == E
    assert L.rmi_length_weight_rows(p, -1, 8, p, p, None) == E
    assert L.rmi_length_weight_rows(p, 4, -1, p, p, None) == E
    assert L.rmi_length_weight_rows(p, 0, 8, p, p, None) == OK
    assert L.rmi_length_weight_finalize(None, 4, p, None) == E
    assert L.rmi_length_weight_finalize(p, 4, None, None) == E
    assert L.rmi_length_weight_finalize(p, -1, p, None) == E
    assert L.rmi_length_weight_finalize(p, 0, p, None) == OK
    gs = lambda **k: L.rmi_grpo_outcome_scaled(*[k.get(n, d) for n, d in (
        ("r", p), ("mask", p), ("B", 4), ("L", 8), ("seg", p), ("G", 2), ("eps", 1e-6), ("norm", 1), ("scale", p),
        ("adv", p), ("ret", p), ("stream", None))])
    for name in ("r", "mask", "seg", "adv", "ret"):
        assert gs(**{name: None}) == E, name
        assert gs(**{name: None, "scale": None}) == E, name
    assert gs(B=-1) == E and gs(L=-1) == E and gs(G=-1) == E
    assert gs(B=0) == OK and gs(B=0, scale=None) == OK
    assert L.rmi_row_div(None, p, 4, 8, None) == E
    assert L.rmi_row_div(p, None, 4, 8, None) == E
    assert L.rmi_row_div(p, p, -1, 8, None) == E and L.rmi_row_div(p, p, 4, -1, None) == E
    assert L.rmi_row_div(p, p, 0, 8, None) == OK


def test_new_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from ragen_amd import torch_ops
    R = torch.ops.ragen_amd
    new = {"kl_reward", "rows_mean", "length_weight_rows", "length_weight_finalize", "grpo_outcome_scaled", "row_div_"}
    assert new <= set(torch_ops.OPS), new - set(torch_ops.OPS)
    assert "!" in str(R.row_div_.default._schema)
    # the existing ops' schemas are unchanged
    assert str(R.grpo_outcome.default._schema) == \
        "ragen_amd::grpo_outcome(Tensor r, Tensor mask, Tensor seg, float eps, bool norm_by_std) -> (Tensor, Tensor)"
    with pytest.raises(NotImplementedError):  # no CPU path
        R.kl_reward(torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.uint8), 0.1, 0)
    with FakeTensorMode():
        B, L = 6, 11
        r = torch.empty(B, L, device="cuda")
        m = torch.empty(B, L, dtype=torch.uint8, device="cuda")
        rew, stats = R.kl_reward(r, r, r, m, 0.1, 3)
        assert rew.shape == (B, L) and rew.dtype == torch.float32
        assert stats.shape == (B, 2) and stats.dtype == torch.float64
        cur = R.rows_mean(stats)
        assert cur.shape == (1,) and cur.dtype == torch.float64
        count, rel = R.length_weight_rows(m)
        assert (count.shape, count.dtype, rel.shape, rel.dtype) == ((B,), torch.int32, (B,), torch.float32)
        assert R.length_weight_finalize(count).shape == (B,)
        seg = torch.empty(3, dtype=torch.int32, device="cuda")
        adv, ret = R.grpo_outcome_scaled(r, m, seg, 1e-6, True, rel)
        assert adv.shape == ret.shape == (B, L)
        adv, ret = R.grpo_outcome_scaled(r, m, seg, 1e-6, True, None)
        assert R.row_div_(adv, rel) is None


def test_length_weight_fixture_equals_the_restatement():
    g = np.load(GOLDEN)
    mask = torch.from_numpy(g["response_mask"].astype(np.int64))
    counts = g["response_mask"].sum(1)
    assert sorted(set(counts.tolist())) == [0, 1, 2, 15, 16, 17, 31, 32, 33, 64] and g["advantages"].shape == (40, 64)
    for a, w in (("advantages", "weighted"), ("grpo_advantages", "grpo_weighted")):
        out = vk.grpo_length_weight(torch.from_numpy(g[a]), mask)
        np.testing.assert_array_equal(out.numpy(), g[w])
    # the f32 add of `sum + 1e-6`: 16 -> 16.000001907, 31 -> 31.000001907, 32 -> 32.0
    plus = (torch.tensor([16, 31, 32]) + 1e-6)
    assert plus.dtype == torch.float32
    np.testing.assert_array_equal(plus.numpy(), np.array([16.000001907, 31.000001907, 32.0], np.float32))
    mean = np.float32(counts.sum()) / np.float32(len(counts))
    row = int(np.flatnonzero(counts == 16)[0])
    np.testing.assert_array_equal(g["weighted"][row], g["advantages"][row] / (np.float32(16.000001907) / mean))
    # GRPO-shaped input: one score per row over the mask, from the stored rewards
    s = torch.from_numpy(g["token_level_rewards"]).sum(-1) / (torch.tensor(1.0) + 1e-6)
    np.testing.assert_array_equal((s.unsqueeze(-1) * torch.from_numpy(g["response_mask"])).numpy(), g["grpo_advantages"])


def test_config_keys_have_the_reference_defaults():
    cfg = default_config()
    assert cfg.grpo_advantage_length_weight is False
    assert cfg.algorithm.use_kl_in_reward is False
    assert cfg.algorithm.kl_penalty == "kl"
    assert dict(cfg.algorithm.kl_ctrl) == {"type": "fixed", "kl_coef": 0.0}
    cfg = default_config(algorithm={"kl_ctrl": {"type": "adaptive", "target_kl": 0.01, "horizon": 100}})
    assert cfg.algorithm.kl_ctrl.type == "adaptive" and cfg.algorithm.kl_ctrl.kl_coef == 0.0
    assert cfg.algorithm.adv_estimator == "gae"  # the other keys are untouched


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rows(rank):  # ragged shards: 3 and 5 rows
    n = (3, 5)[rank]
    stats = torch.arange(2 * n, dtype=torch.float64).view(n, 2) + 100 * rank
    counts = torch.arange(n, dtype=torch.int32) + 10 * rank
    return stats, counts


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    stats, counts = _rows(rank)
    g = rd.gather_row_values(stats, sizes=[3, 5])
    c, off = rd.gather_row_values(counts, with_offset=True)
    q.put((rank, g.numpy(), c.numpy(), off, str(g.dtype), str(c.dtype)))
    dist.destroy_process_group()


def test_gather_row_values_two_rank_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want_s = torch.cat([_rows(0)[0], _rows(1)[0]]).numpy()
    want_c = torch.cat([_rows(0)[1], _rows(1)[1]]).numpy()
    for rank, g, c, off, gdt, cdt in res:
        np.testing.assert_array_equal(g, want_s)     # global row order on both ranks
        np.testing.assert_array_equal(c, want_c)
        assert off == (0, 3)[rank] and gdt == "torch.float64" and cdt == "torch.int32"
    # without a process group: the local rows
    s, _ = _rows(0)
    assert rd.gather_row_values(s) is s and rd.gather_row_values(s, with_offset=True)[1] == 0
