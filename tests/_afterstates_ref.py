"""Shared by tests/test_afterstates_host.py and tests/test_gpu_afterstates.py: the position set of the one-ply
lookahead tests and what the unmodified oracle says about every action of every position.

Expectation for action a of a position held in an ``oracle.bb_game.Env``: ``copy.deepcopy`` it and ``step(a)``.
For a refill move (the third piece of the hand) the copy's engine gets ``_generate = lambda: None`` and
``has_valid_moves = lambda: True`` first, which removes the chance part (the new hand and whether it fits); the
deterministic part -- grid, reward, last_move, holes, centre, blocks, valid moves -- is then read from the copy.
A refill move whose real step terminates is flagged (``chance_end``): its reward is left out of the comparison.

The set is built once per process (both test files share it): 16 host-backend envs, seeds 100-115, stepped in
lockstep with oracle envs, half under random legal play and half under the oracle-side greedy rule, snapshots
before moves 0, 1, 2, 5, 9 and 30 of the games still alive; then crafted positions.
"""
import copy
import functools

import numpy as np
import torch

from oracle import bb_game as O

FIELDS = ("lines", "score", "holes", "filled", "centre", "mobility", "dead", "refill")
DEFAULT_WEIGHTS = {"lines": 100, "score": 0, "holes": -30, "filled": -2, "centre": 0, "mobility": 1,
                   "dead": -100000, "refill": 0}
INT64_MIN = -(2 ** 63)
SNAP_MOVES = (0, 1, 2, 5, 9, 30)


def oracle_action(env, a, want_chance=True):
    """None for an illegal action, else the oracle's deterministic result of action a from env's position."""
    p, r, c = O.Env.action_to_move(a)
    if not env.engine.can_place_piece(p, r, c):
        return None
    refill = sum(env.engine.used) == 2
    cp = copy.deepcopy(env)
    if refill:
        cp.engine._generate = lambda: None
        cp.engine.has_valid_moves = lambda: True
    _, reward, term, _, info = cp.step(a)
    g = cp.engine.grid
    res = {
        "board": O.grid_to_u64(g), "reward": reward, "score": info["last_move"]["score_gained"],
        "lines": info["last_move"]["lines_cleared"], "holes": O.count_holes(g), "centre": O.center_filled(g),
        "filled": O.total_blocks(g), "mobility": len(cp.engine.valid_moves()), "refill": int(refill),
        "dead": int(term), "combo_after": cp.engine.combo, "chance_end": False,
    }
    assert not (refill and term)
    if refill and want_chance:
        res["chance_end"] = bool(copy.deepcopy(env).step(a)[2])
    return res


def value_of(res, weights):
    return sum(int(weights.get(k, 0)) * int(res[k]) for k in FIELDS)


def oracle_greedy(env, weights):
    """(action, value) of the greedy rule on the oracle's features: arg-max over legal actions, lowest on ties."""
    best, best_a = INT64_MIN, 0
    for a in range(192):
        res = oracle_action(env, a, want_chance=False)
        if res is not None and value_of(res, weights) > best:
            best, best_a = value_of(res, weights), a
    return best_a, best


def position_of(env):
    """(board u64, hand word u32, combo, prev u16) of an oracle env, in the C-ABI's packing."""
    e = env.engine
    hand = e.hand[0] | (e.hand[1] << 6) | (e.hand[2] << 12)
    hand |= sum(int(u) << (18 + s) for s, u in enumerate(e.used)) | (int(e.over) << 21)
    centre = int(round((1.0 - env.prev_center) * 16))
    return O.grid_to_u64(e.grid), hand, e.combo, env.prev_holes | (centre << 8)


def make_env(board, hand, used=(False, False, False), over=False, combo=0, prev_holes=0, prev_centre=0):
    """An oracle env holding a crafted position (prev_centre: filled centre cells behind _prev_center_openness)."""
    env = O.Env(seed=0)
    e = env.engine
    e.grid = O.u64_to_grid(board)
    e.hand, e.used, e.over, e.combo = list(hand), list(used), over, combo
    env.prev_holes, env.prev_center = prev_holes, 1.0 - prev_centre / 16.0
    return env


def _bits(cells):
    return sum(1 << (r * 8 + c) for r, c in cells)


def crafted():
    """name -> oracle env.  Piece ids: 0 SINGLE, 1 DOMINO_H, 5 TRIO_H, 17 O, 36 SQUARE_3x3."""
    cross = _bits([(0, c) for c in range(1, 8)] + [(r, 0) for r in range(1, 8)])  # row 0 and column 0 lack (0, 0)
    # two free cells per row and column, never adjacent: a SINGLE fits 16 times, a DOMINO_H nowhere, no
    # placement of the SINGLE completes a line -- every legal move leaves the domino without a place (dead)
    free = [(i, i) for i in range(8)] + [(i, (i + 4) % 8) for i in range(8)]
    tight = (2 ** 64 - 1) & ~_bits(free)
    rng = np.random.default_rng(11)
    while True:  # a half-full board without a full line, with holes and centre cells of its own
        g = (rng.random((8, 8)) < 0.5).astype(int)
        if g.all(1).any() or g.all(0).any():
            continue
        mid = O.grid_to_u64(g.tolist())
        h0, c0 = O.count_holes(g.tolist()), O.center_filled(g.tolist())
        if h0 >= 2 and 4 <= c0 <= 12:
            break
    return {
        "row_and_column": make_env(cross, (0, 1, 17)),
        "combo9": make_env(cross, (0, 5, 17), combo=9),
        "dead": make_env(tight, (0, 1, 36), used=(False, False, True)),
        "game_over": make_env(tight, (17, 1, 36), over=True),
        # prev equal to the board's own holes / centre cells: the hole penalty is on exactly for the moves that
        # add holes, the centre bonus exactly for those that add no centre cell
        "prev_switch": make_env(mid, (0, 1, 5), prev_holes=h0, prev_centre=c0, combo=2),
        "prev_low": make_env(mid, (17, 0, 5), used=(False, False, True), prev_holes=0, prev_centre=0),
        "prev_high": make_env(mid, (0, 5, 1), used=(True, False, True), prev_holes=40, prev_centre=16),
    }


def set_positions(env_batch, envs):
    """Load the oracle envs' positions into a DeviceEnvBatch of the same size (bb_set_state)."""
    pos = [position_of(e) for e in envs]
    env_batch.set_state(board=np.array([p[0] for p in pos], np.uint64), hand=np.array([p[1] for p in pos], np.uint32),
                        combo=np.array([p[2] for p in pos], np.int32),
                        prev_holes=np.array([p[3] & 0xFF for p in pos], np.uint8),
                        prev_center=np.array([p[3] >> 8 for p in pos], np.uint8))


def _played():
    """Snapshots (oracle env copies) of 16 games, the host backend stepped in lockstep with the oracle."""
    from runtime.build import build_host_lib
    from runtime.device_env import DeviceEnvBatch

    build_host_lib(verbose=False)
    n = 16
    seeds = list(range(100, 100 + n))
    host = DeviceEnvBatch(n, seeds, autoreset=False, device="cpu")
    host.reset()
    ora = [O.Env(seed=s) for s in seeds]
    for e in ora:
        e.reset()
    alive = [True] * n
    rng = np.random.default_rng(3)
    snaps = []
    for t in range(max(SNAP_MOVES) + 1):
        st = host.state()
        for i in range(n):  # lockstep: the host backend holds the oracle's position
            b, h, cb, pv = position_of(ora[i])
            assert (int(st["board"][i]), int(st["hand"][i]) & 0x3FFFFF, int(st["combo"][i])) == (b, h, cb), (t, i)
            assert int(st["prev_holes"][i]) | (int(st["prev_center"][i]) << 8) == pv, (t, i)
        if t in SNAP_MOVES:
            snaps += [copy.deepcopy(ora[i]) for i in range(n) if alive[i]]
        if t == max(SNAP_MOVES):
            break
        acts = np.zeros(n, np.int32)
        for i in range(n):
            if not alive[i]:
                continue
            if i % 2 == 0:
                acts[i] = rng.choice(np.nonzero(ora[i].obs()["action_mask"])[0])
            else:
                acts[i] = oracle_greedy(ora[i], DEFAULT_WEIGHTS)[0]
        host.step(torch.from_numpy(acts))
        term = host.terminated.numpy().astype(bool)
        for i in range(n):
            if alive[i]:
                assert bool(ora[i].step(int(acts[i]))[2]) == bool(term[i]), (t, i)
                alive[i] = not term[i]
    host.close()
    return snaps


@functools.lru_cache(maxsize=None)
def reference():
    """The position set and the oracle's expectation, computed once.  Returns a dict of numpy arrays:
    positions board u64 / hand u32 / combo i32 / prev u16 [n]; per action [n, 192]: legal, exp_board u64,
    exp_reward f64, exp_score i32, lines, holes, centre, filled, mobility, dead, refill, chance_end, capped (a
    line-clearing move whose streak factor min(combo' + 1, 8) is capped); names: crafted name -> index."""
    made = crafted()
    envs = _played() + list(made.values())
    n = len(envs)
    names = {k: n - len(made) + j for j, k in enumerate(made)}
    pos = [position_of(e) for e in envs]
    ref = {"envs": envs, "names": names, "n": n,
           "board": np.array([p[0] for p in pos], np.uint64), "hand": np.array([p[1] for p in pos], np.uint32),
           "combo": np.array([p[2] for p in pos], np.int32), "prev": np.array([p[3] for p in pos], np.uint16),
           "legal": np.zeros((n, 192), bool), "exp_board": np.zeros((n, 192), np.uint64),
           "exp_reward": np.full((n, 192), -10.0), "exp_score": np.zeros((n, 192), np.int32),
           "chance_end": np.zeros((n, 192), bool), "capped": np.zeros((n, 192), bool)}
    for k in FIELDS:
        if k != "score":
            ref[k] = np.zeros((n, 192), np.int64)
    for i, env in enumerate(envs):
        ref["exp_board"][i, :] = ref["board"][i]
        for a in range(192):
            res = oracle_action(env, a)
            if res is None:
                continue
            ref["legal"][i, a] = True
            ref["exp_board"][i, a] = res["board"]
            ref["exp_reward"][i, a] = res["reward"]
            ref["exp_score"][i, a] = res["score"]
            ref["chance_end"][i, a] = res["chance_end"]
            ref["capped"][i, a] = res["lines"] > 0 and res["combo_after"] + 1 > 8
            for k in FIELDS:
                if k != "score":
                    ref[k][i, a] = res[k]
    return ref


def expected_aux(ref):
    """The aux word the library must produce, from the oracle's fields (0 for illegal actions)."""
    aux = (1 | (ref["dead"] << 1) | (ref["refill"] << 2) | (ref["lines"] << 8) | (ref["holes"] << 12)
           | (ref["centre"] << 19) | (ref["mobility"] << 24))
    return np.where(ref["legal"], aux, 0).astype(np.uint32)


def expected_greedy(ref, weights):
    """numpy arg-max (lowest index on ties) of the greedy value over the oracle's features: (action, value)."""
    v = sum(int(weights.get(k, 0)) * (ref["exp_score"].astype(np.int64) if k == "score" else ref[k]) for k in FIELDS)
    v = np.where(ref["legal"], v, INT64_MIN)
    a = v.argmax(axis=1)  # numpy returns the first maximum
    a = np.where(ref["legal"].any(axis=1), a, 0)
    return a.astype(np.int32), v[np.arange(len(a)), a].astype(np.int64)


def tensors(ref, dev, idx=None):
    """The positions (all, or those at idx) as the torch tensors runtime.kernels takes."""
    sel = slice(None) if idx is None else idx
    return (torch.from_numpy(ref["board"][sel].view(np.int64).copy()).to(dev),
            torch.from_numpy(ref["hand"][sel].view(np.int32).copy()).to(dev),
            torch.from_numpy(ref["combo"][sel].copy()).to(dev),
            torch.from_numpy(ref["prev"][sel].view(np.int16).copy()).to(dev))


def check_dense(ref, out, idx=None, what=""):
    """All four outputs of an afterstates call against the oracle, every action, legal or not."""
    sel = np.arange(ref["n"]) if idx is None else np.asarray(idx)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(got["board"].view(np.uint64), ref["exp_board"][sel]), f"{what} board"
    assert np.array_equal(got["score_gained"], ref["exp_score"][sel]), f"{what} score_gained"
    assert np.array_equal(got["aux"].view(np.uint32), expected_aux(ref)[sel]), f"{what} aux"
    keep = ~ref["chance_end"][sel]  # fp64 ==, except where the real step's new hand ends the game
    assert np.array_equal(got["reward"][keep], ref["exp_reward"][sel][keep]), f"{what} reward"
