"""The cached Sokoban turn (sokoban_cached_turn_kernel: the 6x6 one-lane layout reading a built board
cache, K fixed at compile time) against the same rollout without a cache
(the general kernel) and against the oracle, bit for bit: the SoA state, the episode record, the
board entries, and the fused last turn's metrics / score / penalty / norm.

Rollouts of 3 turns (fused first turn, plain turn, fused last turn) at B = 4097 (the smallest batch
that keeps the cache: one lane in the last wave) and B = 4224, K in {1, 4, 5, 6, 8} (the dword edges
of the action rows), has_input absent and present on each of the three launches (envs left out of
the building turn included), a budget that cuts a turn short, max_steps reached mid-turn, all four
finalize methods, waves that must fall back to the general turn (an irregular room, an untagged
entry, an action id 9), and a 4x9 batch (36 cells, not 6x6), which stays on the general kernel."""
import numpy as np
import pytest
import torch

import oracle
from ragen_amd import _lib, ops, synthetic
from ragen_amd.env import SokobanBatch
from ragen_amd.env.configs import SokobanEnvConfig
from test_gpu_parity import _host_ep, _t

pytestmark = pytest.mark.gpu
FIELDS = ("num_actions", "flags", "n_turns", "penalty", "turn_reward", "turn_info", "turn_exec")
METHODS = ("identity", "mean", "mean_std", "asym_clip")
T = 3
# has_input present (1) / absent (0) on the three launches of each of three rollouts: the cached
# first turn runs from the second rollout on, so every cached kernel meets both forms
HAS = ((1, 0, 1), (1, 1, 0), (0, 0, 1))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _snap(env):
    s = {k: getattr(env, k).cpu().numpy().copy() for k in ("room_state", "player", "num_env_steps", "boxes_on_target")}
    s.update(_host_ep(env.ep))
    return s


def _match(env, oep, fixed, state, player, nes, bot, ok):
    np.testing.assert_array_equal(env.room_state.cpu().numpy()[ok], state[ok])
    np.testing.assert_array_equal(env.room_fixed.cpu().numpy()[ok], fixed[ok])
    np.testing.assert_array_equal(env.player.cpu().numpy()[ok], player[ok])
    np.testing.assert_array_equal(env.num_env_steps.cpu().numpy()[ok], nes[ok])
    np.testing.assert_array_equal(env.boxes_on_target.cpu().numpy()[ok], bot[ok])
    h = _host_ep(env.ep)
    for k in FIELDS:
        got, want = _bits(h[k]), _bits(np.asarray(getattr(oep, k), h[k].dtype))
        np.testing.assert_array_equal(got[..., ok], want[..., ok], err_msg=k)


def _check_entries(env, fixed, state, player, nes, bot, ok, H, W):
    """Every tagged entry == the boards its room's rows imply: the window words (bit j = cell
    W + j; the bits past the room are padding walls), the player cell, the tag and the counters."""
    ent = env.boards.cpu().numpy()
    tagged = (ent[:, 13] == 1) & ok
    words = np.ascontiguousarray(ent[:, :12]).view(np.uint32)
    win = np.arange(W, H * W)
    sh = (np.uint64(1) << (win - W).astype(np.uint64))

    def board(mask):
        return (mask[:, win].astype(np.uint64) * sh).sum(axis=1).astype(np.uint32)
    pad = np.uint32((~((1 << ((H - 1) * W)) - 1)) & 0xFFFFFFFF)
    np.testing.assert_array_equal(words[tagged, 0], (board(fixed == 0) | pad)[tagged])
    np.testing.assert_array_equal(words[tagged, 1], board(fixed == 2)[tagged])
    np.testing.assert_array_equal(words[tagged, 2], board((state == 3) | (state == 4))[tagged])
    np.testing.assert_array_equal(ent[tagged, 12], (player[:, 0].astype(np.int32) * W + player[:, 1])[tagged])
    np.testing.assert_array_equal(ent[tagged, 14], nes.astype(np.uint8)[tagged])
    np.testing.assert_array_equal(ent[tagged, 15], bot.astype(np.int8).view(np.uint8)[tagged])
    return tagged


def _oracle_finalize(oep, gs, method):
    score, pen = oracle.trajectory_scores(oep)
    seg = np.arange(0, oep.B + 1, gs, dtype=np.int32)
    return oracle.rollout_metrics(oep), score, pen, oracle.group_normalize(score, pen, seg, method)


def _plan(rng, B, K, rollouts, id_hi=8, p_unknown=0.08):
    """Per rollout and turn: (ids i8[B, K], n u8[B], has u8[B] or None)."""
    plan = []
    for r in range(rollouts):
        turns = []
        for t in range(T):
            ids = rng.integers(1, id_hi + 1, size=(B, K))
            ids = np.where(rng.random((B, K)) < p_unknown, 0, ids).astype(np.int8)
            n = rng.integers(0, K + 1, size=B).astype(np.uint8)
            has = (rng.random(B) < 0.75).astype(np.uint8) if HAS[r % 3][t] else None
            turns.append((ids, n, has))
        plan.append(turns)
    return plan


def _run(device, cfg, B, K, plan, cap, method, gs, boards, rooms=None):
    """The plan's rollouts on a fresh batch, with or without the board cache; every turn is held
    to the oracle; -> the per-turn snapshots and per-rollout finalize outputs."""
    H, W = int(cfg.dim_room[0]), int(cfg.dim_room[1])
    env = SokobanBatch(cfg, B, T, K, device)
    assert env.enable_boards() or not boards
    if not boards:
        env.boards = None
    if rooms is None:
        env.reset(synthetic.env_seeds(B))
    else:
        env.load_state(*rooms)
    fixed0 = env.room_fixed.cpu().numpy().copy()
    state0, player0 = env.init_state.cpu().numpy().copy(), env.init_player.cpu().numpy().copy()
    norm = torch.empty(B, dtype=torch.float32, device=device)
    met = torch.empty(B, 4, dtype=torch.float64, device=device)
    sc, pe = torch.empty_like(norm), torch.empty_like(norm)
    fin = ops.finalize_struct(gs, method, norm, met, sc, pe)
    snaps = []
    for turns in plan:
        fixed, state, player = fixed0.copy(), state0.copy(), player0.copy()
        nes, bot = np.zeros(B, np.int32), np.zeros(B, np.int32)
        oep = oracle.Episode(B, T)
        bad = np.zeros(B, bool)
        for t, (ids, n, has) in enumerate(turns):
            keep = (_t(ids, device), _t(n, device), None if has is None else _t(has, device))
            turn = ops.turn_struct(t, *keep, cap, -0.1)
            err = torch.zeros(B, dtype=torch.uint8, device=device)
            use = env.board_struct(_lib.BOARDS_USE) if boards else env.struct()
            if t == 0:
                st = env.board_struct(_lib.BOARDS_USE if env.init_boards_valid else _lib.BOARDS_BUILD) if boards else use
                ops.sokoban_step_turn_first(st, env.ep, turn, env.init_state, env.init_player, err)
                env.init_boards_valid = boards
            elif t == T - 1:
                ops.sokoban_step_turn_finalize(use, env.ep, turn, fin, err)
            else:
                ops.sokoban_step_turn(use, env.ep, turn, err)
            oerr = oracle.sokoban_turn(H, W, int(cfg.num_boxes), int(cfg.max_steps), fixed, state, player, nes, bot,
                                       oep, t, ids, n, has, cap, -0.1)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(err.cpu().numpy() != 0, oerr != 0)
            bad |= oerr != 0
            _match(env, oep, fixed, state, player, nes, bot, ~bad)
            if boards:
                _check_entries(env, fixed, state, player, nes, bot, ~bad, H, W)
            snaps.append((_snap(env), bad.copy()))
        outs = [x.cpu().numpy().copy() for x in (met, sc, pe, norm)]
        if not bad.any():
            for got, want in zip(outs, _oracle_finalize(oep, gs, method)):
                np.testing.assert_array_equal(_bits(got), _bits(want))
        snaps.append((dict(zip(("metrics", "score", "pen", "norm"), outs)), None))
    return env, snaps


def _same(a, b):
    """The cached run's snapshots == the uncached run's (envs the reference raises on left out of
    the per-env fields; the finalize outputs whole)."""
    assert len(a) == len(b)
    for (sa, bad), (sb, _) in zip(a, b):
        for k in sa:
            x, y = _bits(sa[k]), _bits(sb[k])
            if bad is not None and bad.any():
                ok = ~bad
                x, y = (x[ok], y[ok]) if k in ("room_state", "player", "metrics") or x.ndim == 1 else (x[:, ok], y[:, ok])
            np.testing.assert_array_equal(x, y, err_msg=k)


@pytest.mark.parametrize("limit", ["budget", "max_steps"])
@pytest.mark.parametrize("K", [1, 4, 5, 6, 8])
@pytest.mark.parametrize("B", [4097, 4224])
def test_cached_rollouts_vs_uncached_and_oracle(device, B, K, limit):
    # budget: max_actions_per_traj = K + 2 cuts the second or third turn short;
    # max_steps = K + 1 is reached in the middle of the second turn of an env that used the first
    cap, max_steps = (K + 2, 100) if limit == "budget" else (3 * K + 4, K + 1)
    cfg = SokobanEnvConfig(dim_x=6, dim_y=6, num_boxes=1, max_steps=max_steps)
    plan = _plan(np.random.default_rng(1000 * B + 10 * K + (limit == "budget")), B, K, 3)
    env, cached = _run(device, cfg, B, K, plan, cap, "mean_std", 1 if B % 16 else 16, True)
    assert (env.boards.cpu().numpy()[:, 13] == 1).all(), "every generated room stays regular: every entry tagged"
    _, plain = _run(device, cfg, B, K, plan, cap, "mean_std", 1 if B % 16 else 16, False)
    _same(cached, plain)


@pytest.mark.parametrize("method", METHODS)
def test_cached_last_turn_finalize_methods(device, method):
    B, K = 4224, 5
    cfg = SokobanEnvConfig(dim_x=6, dim_y=6, num_boxes=1, max_steps=100)
    plan = _plan(np.random.default_rng(METHODS.index(method)), B, K, 2)
    _, cached = _run(device, cfg, B, K, plan, 10, method, 16, True)
    _, plain = _run(device, cfg, B, K, plan, 10, method, 16, False)
    _same(cached, plain)


@pytest.mark.parametrize("why", ["irregular_room", "untagged_entry", "action_id_9"])
def test_wave_that_falls_back_still_matches(device, why):
    """One env of one wave fails the cached turn's predicate: the wave takes the general turn.
    Every env of the batch still == the oracle (and the error flags where the reference raises)."""
    B, K, H, W = 4224, 5, 6, 6
    cfg = SokobanEnvConfig(dim_x=H, dim_y=W, num_boxes=1, max_steps=100)
    rng = np.random.default_rng(len(why))
    plan = _plan(rng, B, K, 2)
    victim = 64 * 3 + 17  # a lane in the middle of the fourth wave
    rooms = None
    if why == "action_id_9":
        for turns in plan:
            for ids, n, has in turns:
                ids[victim, 0], n[victim] = 9, K
                if has is not None:
                    has[victim] = 1
    else:
        probe = SokobanBatch(cfg, B, T, K, device)
        probe.reset(synthetic.env_seeds(B))
        fixed, state = probe.room_fixed.cpu().numpy().copy(), probe.room_state.cpu().numpy().copy()
        player = probe.player.cpu().numpy().copy()
        if why == "irregular_room":  # an open border cell next to the player's row: not a regular room
            fixed[victim].reshape(H, W)[0, 2] = 1
            state[victim].reshape(H, W)[0, 2] = 1
        rooms = (fixed, state, player)
    env = SokobanBatch(cfg, B, T, K, device)
    assert env.enable_boards()
    env.load_state(*rooms) if rooms is not None else env.reset(synthetic.env_seeds(B))
    fixed0 = env.room_fixed.cpu().numpy().copy()
    state0, player0 = env.init_state.cpu().numpy().copy(), env.init_player.cpu().numpy().copy()
    for r, turns in enumerate(plan):
        fixed, state, player = fixed0.copy(), state0.copy(), player0.copy()
        nes, bot = np.zeros(B, np.int32), np.zeros(B, np.int32)
        oep = oracle.Episode(B, T)
        bad = np.zeros(B, bool)
        for t, (ids, n, has) in enumerate(turns):
            keep = (_t(ids, device), _t(n, device), None if has is None else _t(has, device))
            turn = ops.turn_struct(t, *keep, 10, -0.1)
            err = torch.zeros(B, dtype=torch.uint8, device=device)
            if why == "untagged_entry" and t > 0:
                # the caller's own write of one entry's tag: the env's rows still hold its state
                env.boards[victim, 13] = 0
            if t == 0:
                mode = _lib.BOARDS_USE if env.init_boards_valid else _lib.BOARDS_BUILD
                ops.sokoban_step_turn_first(env.board_struct(mode), env.ep, turn, env.init_state, env.init_player, err)
                env.init_boards_valid = True
            else:
                ops.sokoban_step_turn(env.board_struct(_lib.BOARDS_USE), env.ep, turn, err)
            oerr = oracle.sokoban_turn(H, W, 1, 100, fixed, state, player, nes, bot, oep, t, ids, n, has, 10, -0.1)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(err.cpu().numpy() != 0, oerr != 0)
            bad |= oerr != 0
            _match(env, oep, fixed, state, player, nes, bot, ~bad)
            tagged = _check_entries(env, fixed, state, player, nes, bot, ~bad, H, W)
            # (the general turn untags the envs it steps on the exact path: the victim's wave when
            # its room is irregular or an action id is off the regular path)
            others = np.ones(B, bool)
            others[victim // 64 * 64:(victim // 64 + 1) * 64] = False
            assert tagged[others & ~bad].all()
            if why == "untagged_entry":
                wave = ~others
                wave[victim] = False
                assert tagged[wave].all()
            if why == "irregular_room":
                assert not tagged[victim]


def test_4x9_rooms_stay_on_the_general_kernel(device):
    """36 cells but not 6x6: the launcher keeps the general kernel (which keeps the cache for a
    u32 window), and the rollout == the uncached one and the oracle."""
    B, K, H, W = 4224, 5, 4, 9
    rng = np.random.default_rng(49)
    fixed = np.zeros((B, H, W), np.uint8)
    fixed[:, 1:H - 1, 1:W - 1] = 1
    state = fixed.copy()
    player = np.zeros((B, 2), np.int8)
    inner = [(r, c) for r in range(1, H - 1) for c in range(1, W - 1)]
    for i in range(B):
        (tr, tc), (br, bc), (pr, pc) = (inner[j] for j in rng.choice(len(inner), size=3, replace=False))
        fixed[i, tr, tc] = state[i, tr, tc] = 2
        state[i, br, bc] = 4
        state[i, pr, pc] = 5
        player[i] = (pr, pc)
    rooms = (fixed.reshape(B, H * W), state.reshape(B, H * W), player)
    cfg = SokobanEnvConfig(dim_x=H, dim_y=W, num_boxes=1, max_steps=100)
    plan = _plan(rng, B, K, 2)
    env, cached = _run(device, cfg, B, K, plan, 10, "mean_std", 16, True, rooms)
    assert (env.boards.cpu().numpy()[:, 13] == 1).all()
    _, plain = _run(device, cfg, B, K, plan, 10, "mean_std", 16, False, rooms)
    _same(cached, plain)
