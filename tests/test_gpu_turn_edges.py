"""Edges of the three Sokoban turn launches the benchmark replays (fused first turn, plain turn,
fused last turn) at the smallest batches that reach them, each against the oracle or the separate
launch, bit for bit:
  - the bench's sequence (first turn under BUILD on rollout 1 and USE after, plain USE turns, the
    last turn fused with the finalize) for 3 rollouts, T in {3, 5, 8, 9} (9: the record loop past
    the 8 turns loaded up front), has_input patterns that leave envs out of the first and the last
    turn, 10 % unknown action ids; every field after every turn, every env's whole room_state row;
  - the error flags with 1 % irregular rooms and action ids outside 1..8, with and without an err
    tensor;
  - the fused last turn against rmi_rollout_finalize and the oracle's normalisation for all four
    methods and every group size a wave holds, with and without the optional outputs;
  - FrozenLake's fused last turn, which shares the finalize.
B = 4112 (257 groups of 16: the last live wave has 16 live lanes, its workgroup's second wave
none) and B = 4160 (65 x 64) take the one-lane-per-env layout with the board cache, B = 80 the
4-lane layout."""
import numpy as np
import pytest
import torch

import oracle
from ragen_amd import _lib, ops, synthetic
from ragen_amd.env import FrozenLakeBatch, SokobanBatch
from ragen_amd.env.configs import FrozenLakeEnvConfig, SokobanEnvConfig
from test_gpu_parity import _host_ep, _irregular_rooms, _t

pytestmark = pytest.mark.gpu
FIELDS = ("num_actions", "flags", "n_turns", "penalty", "turn_reward", "turn_info", "turn_exec")
METHODS = ("identity", "mean", "mean_std", "asym_clip")
CFG = SokobanEnvConfig(dim_x=6, dim_y=6, num_boxes=1, max_steps=100)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _match(env, oep, fixed, state, player, nes, bot, ok=None):
    ok = np.ones(env.B, bool) if ok is None else ok
    np.testing.assert_array_equal(env.room_state.cpu().numpy()[ok], state[ok])
    np.testing.assert_array_equal(env.room_fixed.cpu().numpy()[ok], fixed[ok])
    np.testing.assert_array_equal(env.player.cpu().numpy()[ok], player[ok])
    np.testing.assert_array_equal(env.num_env_steps.cpu().numpy()[ok], nes[ok])
    np.testing.assert_array_equal(env.boxes_on_target.cpu().numpy()[ok], bot[ok])
    h = _host_ep(env.ep)
    for k in FIELDS:
        got, want = h[k], getattr(oep, k)
        if got.dtype.kind == "f":  # bit for bit
            got, want = _bits(got), _bits(np.asarray(want, got.dtype))
        if got.ndim == 2:
            np.testing.assert_array_equal(got[:, ok], want[:, ok], err_msg=k)
        else:
            np.testing.assert_array_equal(got[ok], want[ok], err_msg=k)


def _oracle_finalize(oep, gs, method):
    """-> (metrics, score, pen, norm) of the oracle's episode record."""
    score, pen = oracle.trajectory_scores(oep)
    seg = np.arange(0, oep.B + 1, gs, dtype=np.int32)
    return oracle.rollout_metrics(oep), score, pen, oracle.group_normalize(score, pen, seg, method)


@pytest.mark.parametrize("T", [3, 5, 8, 9])
@pytest.mark.parametrize("B", [4112, 80])
def test_bench_sequence_vs_oracle(device, B, T):
    K, CAP, GS = 5, 10, 16
    env = SokobanBatch(CFG, B, T, K, device)
    boards = env.enable_boards()
    assert boards == (B > 4096)
    env.reset(synthetic.env_seeds(B))
    fixed0 = env.room_fixed.cpu().numpy().copy()
    state0, player0 = env.room_state.cpu().numpy().copy(), env.player.cpu().numpy().copy()
    rng = np.random.default_rng(1000 * T + B)
    norm = torch.empty(B, dtype=torch.float32, device=device)
    met = torch.empty(B, 4, dtype=torch.float64, device=device)
    sc, pe = torch.empty_like(norm), torch.empty_like(norm)
    fin = ops.finalize_struct(GS, "mean_std", norm, met, sc, pe)
    for rollout in range(3):
        fixed, state, player = fixed0.copy(), state0.copy(), player0.copy()
        nes, bot = np.zeros(B, np.int32), np.zeros(B, np.int32)
        oep = oracle.Episode(B, T)
        ids, n = synthetic.rollout_actions(B, T, K, 1, 4, seed=50 + rollout)
        ids = np.where(rng.random(ids.shape) < 0.1, 0, ids).astype(np.int8)  # unknown action names
        has = (rng.random((T, B)) < 0.75).astype(np.uint8)
        for t in range(T):
            # the first and the last turn leave envs out; in between, every second turn feeds the
            # envs whose DONE bit is clear
            h_in = has[t] if (t == 0 or t == T - 1 or t % 2 == 0) else None
            keep = (_t(ids[t], device), _t(n[t], device), None if h_in is None else _t(h_in, device))
            turn = ops.turn_struct(t, *keep, CAP, -0.1)
            use = env.board_struct(_lib.BOARDS_USE) if boards else env.struct()
            if t == 0:
                st = env.board_struct(_lib.BOARDS_USE if env.init_boards_valid else _lib.BOARDS_BUILD) if boards else use
                ops.sokoban_step_turn_first(st, env.ep, turn, env.init_state, env.init_player)
                env.init_boards_valid = boards
            elif t == T - 1:
                ops.sokoban_step_turn_finalize(use, env.ep, turn, fin)
            else:
                ops.sokoban_step_turn(use, env.ep, turn)
            oracle.sokoban_turn(6, 6, 1, 100, fixed, state, player, nes, bot, oep, t, ids[t], n[t], h_in, CAP, -0.1)
            torch.cuda.synchronize()
            _match(env, oep, fixed, state, player, nes, bot)  # (every env's whole room_state row included)
        for got, want in zip((met, sc, pe, norm), _oracle_finalize(oep, GS, "mean_std")):
            np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(want))
        if boards:
            assert (env.boards.cpu().numpy()[:, 13] == 1).all()


@pytest.mark.parametrize("B", [4112, 80])
def test_error_flags_with_and_without_err(device, B):
    """1 % irregular rooms and action ids outside 1..8: some waves take the exact path.  The flags
    == the oracle's, and the state with err == the state without."""
    T, K, H, W = 4, 6, 6, 6
    outs = []
    for with_err in (True, False):
        rng = np.random.default_rng(B + 11)
        env = SokobanBatch(SokobanEnvConfig(dim_x=H, dim_y=W, num_boxes=1, max_steps=12), B, T, K, device)
        env.enable_boards()
        env.reset(synthetic.env_seeds(B))
        fixed = env.room_fixed.cpu().numpy().copy()
        state = env.room_state.cpu().numpy().copy()
        player = env.player.cpu().numpy().copy()
        idx = np.nonzero(rng.random(B) < 0.01)[0]
        if not len(idx):
            idx = np.array([B // 2])
        f2, s2, p2 = fixed[idx].copy(), state[idx].copy(), player[idx].copy()
        _irregular_rooms(rng, len(idx), H, W, f2, s2, p2)
        fixed[idx], state[idx], player[idx] = f2, s2, p2
        env.load_state(fixed, state, player)
        nes, bot = np.zeros(B, np.int32), np.zeros(B, np.int32)
        oep = oracle.Episode(B, T)
        bad = np.zeros(B, bool)
        for t in range(T):
            ids = rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, -1], size=(B, K),
                             p=[0.05] + [0.11] * 8 + [0.03, 0.04]).astype(np.int8)
            if t == 2:  # a turn on the regular path only: the cached waves step from their entries
                ids = np.clip(ids, 1, 8).astype(np.int8)
            n = rng.integers(0, K + 1, size=B).astype(np.uint8)
            err = torch.zeros(B, dtype=torch.uint8, device=device) if with_err else None
            env.step_turn(t, _t(ids, device), _t(n, device), None, 9, -0.1, err)
            oerr = oracle.sokoban_turn(H, W, 1, 12, fixed, state, player, nes, bot, oep, t, ids, n, None, 9, -0.1)
            torch.cuda.synchronize()
            if with_err:
                np.testing.assert_array_equal(err.cpu().numpy() != 0, oerr != 0)
            bad |= oerr != 0
            _match(env, oep, fixed, state, player, nes, bot, ~bad)
        assert bad.any() and not bad.all()
        outs.append((env.room_state.clone(), env.player.clone(), env.num_env_steps.clone(), env.boxes_on_target.clone(),
                     env.ep.arena.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def _rollout_to_last(make, step, B, T, device, seed):
    """A fresh batch stepped through turns 0..T-2 (two envs in three fed each turn)."""
    K = 5
    ids, n = synthetic.rollout_actions(B, T, K, 1, 4, seed=seed)
    rng = np.random.default_rng(seed)
    has = (rng.random((T, B)) < 0.67).astype(np.uint8)
    b = make(B, T, K)
    b.reset(synthetic.env_seeds(B))
    for t in range(T - 1):
        step(b, ops.turn_struct(t, _t(ids[t], device), _t(n[t], device), _t(has[t], device), 10, -0.1))
    return b, (_t(ids[T - 1], device), _t(n[T - 1], device), _t(has[T - 1], device))


def _check_last_turn(device, B, T, sizes, methods, make, step, step_fin, state_of, seed):
    """The fused last turn from one snapshot of the batch before it: == the plain turn + the
    separate rmi_rollout_finalize launch, and == the oracle's finalize of the record it leaves."""
    b, keep = _rollout_to_last(make, step, B, T, device, seed)
    torch.cuda.synchronize()
    snap = [x.clone() for x in state_of(b)] + [b.ep.arena.clone()]
    turn = ops.turn_struct(T - 1, *keep, 10, -0.1)

    def restore():
        for x, s in zip(state_of(b) + [b.ep.arena], snap):
            x.copy_(s)

    def outputs(which):
        o = {"norm": torch.full((B,), 7.0, dtype=torch.float32, device=device)}
        if which == "all":
            o["metrics"] = torch.full((B, 4), 7.0, dtype=torch.float64, device=device)
            o["score"] = torch.full((B,), 7.0, dtype=torch.float32, device=device)
            o["pen"] = torch.full((B,), 7.0, dtype=torch.float32, device=device)
        return o

    # the reference once: the plain turn, then the separate finalize launch per (size, method)
    restore()
    step(b, turn)
    torch.cuda.synchronize()
    after = [x.clone() for x in state_of(b)] + [b.ep.arena.clone()]
    oep = oracle.Episode(B, T)
    h = _host_ep(b.ep)
    for k in FIELDS:
        getattr(oep, k)[...] = h[k]
    for gs in sizes:
        seg = torch.arange(0, B + 1, gs, dtype=torch.int32, device=device)
        for method in methods:
            ref = outputs("all")
            ops.rollout_finalize(b.ep, seg, method, ref["norm"], ref["metrics"], ref["score"], ref["pen"])
            torch.cuda.synchronize()
            want = dict(zip(("metrics", "score", "pen", "norm"), _oracle_finalize(oep, gs, method)))
            for which in ("all", "norm"):
                restore()
                o = outputs(which)
                step_fin(b, turn, ops.finalize_struct(gs, method, o["norm"], o.get("metrics"), o.get("score"),
                                                      o.get("pen")))
                torch.cuda.synchronize()
                for x, y in zip(state_of(b) + [b.ep.arena], after):
                    assert torch.equal(x, y), (gs, method, which)
                for k, got in o.items():
                    g = _bits(got.cpu().numpy())  # NaNs compared by bit pattern
                    np.testing.assert_array_equal(g, _bits(ref[k].cpu().numpy()), err_msg=f"{k} {gs} {method} {which}")
                    np.testing.assert_array_equal(g, _bits(want[k]), err_msg=f"oracle {k} {gs} {method} {which}")


def _sok_make(device):
    def make(B, T, K):
        b = SokobanBatch(CFG, B, T, K, device)
        b.enable_boards()
        return b
    return make


def _sok_struct(b):
    return b.board_struct(_lib.BOARDS_USE if b._boards_valid else _lib.BOARDS_BUILD) if b.boards is not None \
        else b.struct()


def _sok_step(b, turn):
    ops.sokoban_step_turn(_sok_struct(b), b.ep, turn)
    b._boards_valid = b.boards is not None


def _sok_step_fin(b, turn, fin):
    ops.sokoban_step_turn_finalize(_sok_struct(b), b.ep, turn, fin)
    b._boards_valid = b.boards is not None


def _sok_state(b):
    return [b.room_state, b.player, b.num_env_steps, b.boxes_on_target] + ([b.boards] if b.boards is not None else [])


@pytest.mark.parametrize("B,T,sizes", [(4160, 5, (1, 2, 4, 8, 16, 32, 64)), (4160, 9, (16, 64)), (80, 5, (1, 4, 16))])
def test_fused_last_turn_vs_finalize_and_oracle(device, B, T, sizes):
    _check_last_turn(device, B, T, sizes, METHODS, _sok_make(device), _sok_step, _sok_step_fin, _sok_state, seed=B + T)


def test_frozenlake_fused_last_turn_vs_finalize_and_oracle(device):
    def make(B, T, K):
        return FrozenLakeBatch(FrozenLakeEnvConfig(), B, T, K, device)

    def step(b, turn):
        ops.frozenlake_step_turn(b.struct(), b.ep, turn)

    def step_fin(b, turn, fin):
        ops.frozenlake_step_turn_finalize(b.struct(), b.ep, turn, fin)

    _check_last_turn(device, 80, 5, (1, 4, 16), ("identity", "mean_std"), make, step, step_fin,
                     lambda b: [b.desc, b.s, b.rng], seed=7)
