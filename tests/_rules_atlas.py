"""The rules atlas (not a test module): crafted positions that pin every piece, every anchor and every 0-6-line
clear to the unmodified oracle, shared by tests/test_rules_atlas_host.py and tests/test_gpu_rules_atlas.py.

The score, combo, reward and info rules live in one header (csrc/bb_rules.h) that the HIP kernels and the host
backend both compile, so "HIP equals the host backend" no longer checks them: only the oracle can.  Positions that
play produces stop at 3-4 lines per move and a combo of about 5, below the streak cap min(combo + 1, 8) and below
the line cap min(lines, 4).  The positions here are built instead:

Line-clear atlas: for every piece id p and every anchor (r, c) legal on an empty board (1,623 pairs), with F the
footprint, five boards by the lines that are pre-filled -- all of rows(F) and cols(F); rows(F); cols(F); the first
row and the last column; none -- with F removed from them (no line is full before the move, the placement completes
exactly the chosen ones), random noise outside rows(F) and cols(F), and the noise undone where it would complete a
line.  Over the position index i cycle: the slot that holds p (i % 3), the used pattern (none / one other / both
others used; the last is a refill move, so the env's PCG64 stream must be default_rng(SEED0 + i)'s), the combo
({0, 1, 5, 6, 7, 8, 20}: both sides of the streak cap), max_combo (combo or combo + 3), the score (a multiple of
2**31 - 7: 64-bit accumulation), the episode counters, prev_holes / prev_centre (random).  Every fourth position is
of the dead-end family: noise density 0.6 and SQUARE_3x3 as the other two pieces, so many of these moves end the game.

Blocker boards, for the legality program: the 64 one-cell boards under 13 hands that hold all 37 pieces (the illegal
in-bounds anchors of a piece are exactly the cell minus each of its offsets), and for every (piece, anchor) the board
that is full except F (exactly one anchor of the piece is legal).

Every expectation comes from ``oracle.bb_game``: ``_afterstates_ref.make_env`` (plus engine.max_combo / score /
rng), ``env.step(a)``, ``oracle_action`` for the one-ply record, ``env.obs()["action_mask"]`` for masks.  The
coverage conditions are asserted here on the oracle's results alone.  Everything is built once per process.
"""
import functools

import numpy as np
import torch

import _afterstates_ref as R
from _crowded import mask_bits
from oracle import bb_game as O
from oracle import philox

COMBOS = (0, 1, 5, 6, 7, 8, 20)
VARIANTS = ("rows+cols", "rows", "cols", "first row+last col", "none")
USED_PATTERNS = ("none used", "one other used", "both others used")
SCORE_UNIT = 2 ** 31 - 7
SEED0 = 9000
POLICY_SEED = 0xB10C
ROLLOUT_STEPS = 3
SQUARE_3x3 = 36
CUSTOM_REWARDS = {"line_clear_base": 2.5, "block_placed": 0.03, "game_over_penalty": -3.0, "hole_penalty": -0.25,
                  "center_bonus": 0.7, "combo_multiplier_bonus": 1.25, "survival_bonus": 0.0625}
GREEDY_WEIGHTS = {"score": {"score": 1}, "lines-holes": {"lines": 1, "holes": -1}}
INFO_FIELDS = ("score", "score_gained", "last_cm", "last_lines", "last_blocks", "max_combo", "moves", "lines",
               "blocks", "holes", "filled", "flags")
STATE_FIELDS = ("board", "combo", "max_combo", "score", "moves", "lines", "blocks", "prev_holes", "prev_center",
                "hand")


def pairs():
    """Every (piece id, row, col) that is legal on an empty board, piece-major."""
    out = [(p, r, c) for p in range(O.NUM_PIECES) for r in range(O.BOARD - O.PIECE_H[p] + 1)
           for c in range(O.BOARD - O.PIECE_W[p] + 1)]
    assert len(out) == 1623
    return out


def _footprint(p, r, c):
    cells = [(r + dr, c + dc) for dr, dc in O.PIECE_CELLS[p]]
    return cells, sorted({x for x, _ in cells}), sorted({y for _, y in cells})


def _atlas_board(rng, p, r, c, variant, density):
    cells, rows, cols = _footprint(p, r, c)
    fill_rows, fill_cols = ((rows, cols), (rows, []), ([], cols), (rows[:1], cols[-1:]), ([], []))[variant]
    g = np.zeros((8, 8), bool)
    g[fill_rows, :] = True
    g[:, fill_cols] = True
    for cell in cells:
        g[cell] = False
    noise = rng.random((8, 8)) < density
    noise[rows, :] = False
    noise[:, cols] = False
    for axis in (1, 0):  # undo the noise in any row, then any column, that it would complete
        for k in np.nonzero((g | noise).all(axis=axis))[0]:
            line = noise[k, :] if axis == 1 else noise[:, k]
            line[rng.choice(np.nonzero(line)[0])] = False
    g |= noise
    assert not g.all(1).any() and not g.all(0).any()  # the reference never holds a full line
    after = g.copy()
    for cell in cells:
        assert not after[cell]
        after[cell] = True
    assert sorted(np.nonzero(after.all(1))[0]) == sorted(fill_rows)  # exactly the chosen lines complete
    assert sorted(np.nonzero(after.all(0))[0]) == sorted(fill_cols)
    return O.grid_to_u64(g.astype(int).tolist())


@functools.lru_cache(maxsize=None)
def positions():
    """The atlas positions as numpy columns (no oracle involved yet): what bb_set_state / bb_positions take, the
    crafted action, and what names a position in a failure message."""
    rng = np.random.default_rng(20240607)
    pr = pairs()
    n = len(pr) * len(VARIANTS)
    pos = {"n": n, "piece": np.zeros(n, np.int32), "row": np.zeros(n, np.int32), "col": np.zeros(n, np.int32),
           "variant": np.arange(n, dtype=np.int32) % 5, "slot": np.arange(n, dtype=np.int32) % 3,
           "pattern": (np.arange(n, dtype=np.int32) // 3) % 3, "dead_end": np.arange(n) % 4 == 0,
           "board": np.zeros(n, np.uint64), "ids": np.zeros((n, 3), np.int32), "used": np.zeros((n, 3), bool),
           "combo": np.array([COMBOS[i % 7] for i in range(n)], np.int32),
           "score": (np.arange(n, dtype=np.int64) % 11) * SCORE_UNIT,
           "moves": np.arange(n, dtype=np.int32) % 13, "lines": np.arange(n, dtype=np.int32) % 17,
           "blocks": np.arange(n, dtype=np.int32) % 19,
           "prev_holes": rng.integers(0, 9, n).astype(np.uint8), "prev_center": rng.integers(0, 17, n).astype(np.uint8),
           "seed": SEED0 + np.arange(n, dtype=np.int64)}
    pos["max_combo"] = pos["combo"] + 3 * ((np.arange(n, dtype=np.int32) // 7) % 2)
    for i in range(n):
        p, r, c = pr[i // 5]
        slot, pattern = int(pos["slot"][i]), int(pos["pattern"][i])
        pos["piece"][i], pos["row"][i], pos["col"][i] = p, r, c
        dead_end = bool(pos["dead_end"][i])
        pos["board"][i] = _atlas_board(rng, p, r, c, i % 5, 0.6 if dead_end else (0.1, 0.25, 0.4)[(i // 4) % 3])
        others = rng.integers(0, O.NUM_PIECES, 2)
        pos["ids"][i] = SQUARE_3x3 if dead_end else others[0]
        pos["ids"][i, (slot + 1) % 3] = SQUARE_3x3 if dead_end else others[1]
        pos["ids"][i, slot] = p
        if pattern == 1:
            pos["used"][i, (slot + 1 + (i // 9) % 2) % 3] = True
        elif pattern == 2:
            pos["used"][i] = True
            pos["used"][i, slot] = False
    pos["action"] = (pos["slot"] * 64 + pos["row"] * 8 + pos["col"]).astype(np.int32)
    pos["hand"] = _hand_words(pos["ids"], pos["used"])
    pos["prev"] = (pos["prev_holes"].astype(np.uint16) | (pos["prev_center"].astype(np.uint16) << 8))
    return pos


def _hand_words(ids, used, over=None, has32=None):
    ids, used = np.asarray(ids, np.uint32), np.asarray(used, np.uint32)
    h = ids[:, 0] | (ids[:, 1] << 6) | (ids[:, 2] << 12) | (used[:, 0] << 18) | (used[:, 1] << 19) | (used[:, 2] << 20)
    if over is not None:
        h = h | (np.asarray(over, np.uint32) << 21)
    if has32 is not None:
        h = h | (np.asarray(has32, np.uint32) << 22)
    return h.astype(np.uint32)


def describe(pos, i):
    """The name of atlas position i for a failure message."""
    i = int(i)
    return (f"position {i}: piece {O.PIECE_NAMES[pos['piece'][i]]} ({pos['piece'][i]}) at anchor "
            f"({pos['row'][i]}, {pos['col'][i]}), variant '{VARIANTS[pos['variant'][i]]}', slot {pos['slot'][i]}, "
            f"{USED_PATTERNS[pos['pattern'][i]]}, combo {pos['combo'][i]}, max_combo {pos['max_combo'][i]}"
            f"{', dead-end family' if pos['dead_end'][i] else ''}")


def oracle_env(pos, i, reward_config=None):
    """A fresh oracle env that holds atlas position i."""
    env = R.make_env(int(pos["board"][i]), [int(x) for x in pos["ids"][i]], used=[bool(u) for u in pos["used"][i]],
                     combo=int(pos["combo"][i]), prev_holes=int(pos["prev_holes"][i]),
                     prev_centre=int(pos["prev_center"][i]))
    e = env.engine
    e.max_combo, e.score = int(pos["max_combo"][i]), int(pos["score"][i])
    e.moves, e.lines, e.blocks = int(pos["moves"][i]), int(pos["lines"][i]), int(pos["blocks"][i])
    env.seed_value = int(pos["seed"][i])  # what a reset re-seeds with (block_blast_env.py:212-215)
    e.rng = np.random.default_rng(env.seed_value)
    if reward_config:
        env.rw.update(reward_config)
    return env


def _post_state(env, out, i):
    g = env.engine
    s = g.rng.bit_generator.state
    out["board"][i] = O.grid_to_u64(g.grid)
    out["combo"][i], out["max_combo"][i], out["score"][i] = g.combo, g.max_combo, g.score
    out["moves"][i], out["lines"][i], out["blocks"][i] = g.moves, g.lines, g.blocks
    out["prev_holes"][i] = env.prev_holes
    out["prev_center"][i] = int(round((1.0 - env.prev_center) * 16))
    out["ids"][i], out["used"][i], out["over"][i] = g.hand, g.used, g.over
    out["rng_hi"][i], out["rng_lo"][i] = s["state"]["state"] >> 64, s["state"]["state"] & (2 ** 64 - 1)
    out["has32"][i], out["uinteger"][i] = s["has_uint32"], s["uinteger"]


def _state_columns(n):
    return {"board": np.zeros(n, np.uint64), "combo": np.zeros(n, np.int32), "max_combo": np.zeros(n, np.int32),
            "score": np.zeros(n, np.int64), "moves": np.zeros(n, np.int32), "lines": np.zeros(n, np.int32),
            "blocks": np.zeros(n, np.int32), "prev_holes": np.zeros(n, np.uint8), "prev_center": np.zeros(n, np.uint8),
            "ids": np.zeros((n, 3), np.int32), "used": np.zeros((n, 3), bool), "over": np.zeros(n, bool),
            "rng_hi": np.zeros(n, np.uint64), "rng_lo": np.zeros(n, np.uint64), "has32": np.zeros(n, bool),
            "uinteger": np.zeros(n, np.uint64)}


def _finish_state(st):
    st["hand"] = _hand_words(st["ids"], st["used"], st["over"], st["has32"])
    return st


def reference(custom=False):
    return _reference(bool(custom))  # one cache entry per config, however the argument was spelt


@functools.lru_cache(maxsize=None)
def _reference(custom):
    """What the oracle says about the crafted move of every atlas position, under the default reward config or
    under CUSTOM_REWARDS (then without the one-ply record).  Returns a dict of numpy arrays over the positions:
    reward f64, term, move_lines; info: dict of INFO_FIELDS; post: the state after the move (no auto-reset) with
    the packed hand word; post_mask [n, 192]; legal [n, 192] (the mask before the move); one: the one-ply record of
    the crafted action (board, reward, score, lines, holes, centre, filled, mobility, dead, refill); chance_end."""
    pos = positions()
    n = pos["n"]
    ref = {"pos": pos, "n": n, "reward": np.zeros(n), "term": np.zeros(n, bool), "move_lines": np.zeros(n, np.int64),
           "info": {k: np.zeros(n, np.int64) for k in INFO_FIELDS}, "post": _state_columns(n),
           "post_mask": np.zeros((n, 192), bool), "legal": np.zeros((n, 192), bool), "envs": []}
    one = {k: np.zeros(n, np.int64) for k in ("score", "lines", "holes", "centre", "filled", "mobility", "dead",
                                              "refill")}
    one["board"], one["reward"] = np.zeros(n, np.uint64), np.zeros(n)
    for i in range(n):
        env = oracle_env(pos, i, CUSTOM_REWARDS if custom else None)
        a = int(pos["action"][i])
        if not custom:
            ref["legal"][i] = env.obs()["action_mask"].astype(bool)
            res = R.oracle_action(env, a, want_chance=False)
            assert res is not None, describe(pos, i)
            for k in one:
                one[k][i] = res[k]
        _, reward, term, _, info = env.step(a)
        assert not info["invalid_action"], describe(pos, i)
        last = info["last_move"]
        ref["reward"][i], ref["term"][i], ref["move_lines"][i] = reward, term, last["lines_cleared"]
        inf = ref["info"]
        inf["score"][i], inf["score_gained"][i], inf["last_cm"][i] = info["score"], last["score_gained"], last["combo_multiplier"]
        inf["last_lines"][i], inf["last_blocks"][i] = last["lines_cleared"], last["blocks_placed"]
        inf["max_combo"][i], inf["moves"][i], inf["lines"][i] = info["max_combo"], info["moves"], info["lines_cleared"]
        inf["blocks"][i], inf["holes"][i] = info["blocks_placed"], info["holes"]
        inf["filled"][i] = O.total_blocks(env.engine.grid)
        assert inf["filled"][i] / 64 == info["board_fill"]
        inf["flags"][i] = 4 | (2 if term else 0)  # bbvec.h: bit 1 terminated, bit 2 has last_move
        _post_state(env, ref["post"], i)
        ref["post_mask"][i] = env.engine.action_mask().reshape(-1)
        if not custom:
            ref["envs"].append(env)  # rollout_reference steps them on
    _finish_state(ref["post"])
    if not custom:
        ref["one"] = one
        # the real step of a refill move ended the game: its one-ply reward (game_over = False) is left out
        ref["chance_end"] = (one["refill"] == 1) & ref["term"]
        _assert_coverage(ref)
    return ref


def _assert_coverage(ref):
    """On the oracle's results alone: an edit of this module cannot hollow the set out unnoticed."""
    pos, n = ref["pos"], ref["n"]
    assert n <= 8500
    seen = set(zip(pos["piece"].tolist(), pos["row"].tolist(), pos["col"].tolist()))
    assert seen == set(pairs()), "not every (piece, anchor) pair is present"
    assert np.array_equal(pos["action"], pos["slot"] * 64 + pos["row"] * 8 + pos["col"])
    lines = ref["move_lines"]
    hist = np.bincount(lines, minlength=7)
    assert len(hist) == 7 and (hist >= 100).all(), f"lines histogram {hist.tolist()}"
    combo_after = ref["post"]["combo"]
    capped = (lines > 0) & (combo_after > 7)  # min(combo' + 1, 8) binds
    assert capped.sum() >= 1000, int(capped.sum())
    assert ref["term"].sum() >= 100, int(ref["term"].sum())
    for k in range(3):
        share = float((pos["pattern"] == k).mean())
        assert 0.32 < share < 0.35, (USED_PATTERNS[k], share)
    assert np.array_equal(ref["one"]["refill"] == 1, pos["pattern"] == 2)
    for cb in COMBOS:
        for k in range(1, 7):
            assert ((pos["combo"] == cb) & (lines == k)).any(), f"no {k}-line move at combo {cb}"
    # both the max_combo update and the no-update case, at a capped streak
    assert (capped & (ref["post"]["max_combo"] > pos["max_combo"])).any()
    assert (capped & (ref["post"]["max_combo"] == pos["max_combo"])).any()
    ref["capped"] = capped


def summary(ref):
    """The counts a test prints: positions, lines histogram, capped, terminated, chance_end."""
    return (f"{ref['n']} positions; lines per move 0..6: {np.bincount(ref['move_lines'], minlength=7).tolist()}; "
            f"{int(ref['capped'].sum())} line-clearing moves at a capped streak; {int(ref['term'].sum())} game-ending "
            f"moves; {int(ref['chance_end'].sum())} chance_end")


@functools.lru_cache(maxsize=None)
def rollout_reference():
    """ROLLOUT_STEPS steps with auto-reset from every atlas position under the oracle: the crafted action first,
    then the Philox policy's (oracle/philox.py) on the oracle's masks.  Per step [T, n]: action, reward (f32), term,
    lines, mask [T, n, 192] (after the step and any reset); next_action [n]; final: the state after the last step."""
    ref = reference()
    n, T = ref["n"], ROLLOUT_STEPS
    envs = ref.pop("envs")  # stepped on from here: nobody else may use them
    out = {"action": np.zeros((T, n), np.int32), "reward": np.zeros((T, n), np.float32), "term": np.zeros((T, n), bool),
           "lines": np.zeros((T, n), np.int64), "mask": np.zeros((T, n, 192), bool), "final": _state_columns(n)}
    cur = ref["pos"]["action"].astype(np.int32)
    for t in range(T):
        out["action"][t] = cur
        for i, env in enumerate(envs):
            if t == 0:
                r, term, lines = ref["reward"][i], ref["term"][i], ref["move_lines"][i]
            else:
                _, r, term, _, inf = env.step(int(cur[i]))
                lines = inf.get("last_move", {}).get("lines_cleared", 0)
            out["reward"][t, i], out["term"][t, i], out["lines"][t, i] = np.float32(r), term, lines
            if term:  # wrappers.py:97-102: the vec env resets (re-seeded with seed_value)
                env.reset()
            out["mask"][t, i] = env.engine.action_mask().reshape(-1)
        cur = philox.random_policy(out["mask"][t], POLICY_SEED, t + 1)
    out["next_action"] = cur
    for i, env in enumerate(envs):
        _post_state(env, out["final"], i)
    _finish_state(out["final"])
    return out


def greedy_subset():
    """The cheap subset for the greedy / plan entry points: every 9th of the both-others-used positions."""
    return np.nonzero(positions()["pattern"] == 2)[0][::9]


@functools.lru_cache(maxsize=None)
def greedy_reference():
    """name of GREEDY_WEIGHTS -> (action, value) over greedy_subset(): the arg-max over the one piece's legal
    anchors of the oracle's features, lowest action on ties."""
    pos = positions()
    idx = greedy_subset()
    out = {k: (np.zeros(len(idx), np.int32), np.full(len(idx), R.INT64_MIN, np.int64)) for k in GREEDY_WEIGHTS}
    for j, i in enumerate(idx):
        env = oracle_env(pos, i)
        for a in np.nonzero(env.obs()["action_mask"])[0]:
            res = R.oracle_action(env, int(a), want_chance=False)
            for k, w in GREEDY_WEIGHTS.items():
                v = R.value_of(res, w)
                if v > out[k][1][j]:
                    out[k][0][j], out[k][1][j] = a, v
    return out


@functools.lru_cache(maxsize=None)
def blockers():
    """The blocker boards: board u64 / hand u32 [m], legal [m, 192] from the oracle, and a label per board."""
    boards, hands, labels = [], [], []
    covering = [tuple((3 * k + j) % O.NUM_PIECES for j in range(3)) for k in range(13)]  # 13 hands, all 37 pieces
    assert {p for h in covering for p in h} == set(range(O.NUM_PIECES))
    for cell in range(64):
        for h in covering:
            boards.append(1 << cell)
            hands.append(h)
            labels.append(f"one filled cell ({cell // 8}, {cell % 8}), hand {h}")
    n_single = len(boards)
    full = 2 ** 64 - 1
    for p, r, c in pairs():
        cells, _, _ = _footprint(p, r, c)
        boards.append(full & ~sum(1 << (x * 8 + y) for x, y in cells))
        hands.append(((p - 1) % O.NUM_PIECES, p, (p + 1) % O.NUM_PIECES))
        labels.append(f"full except {O.PIECE_NAMES[p]} ({p}) at ({r}, {c})")
    m = len(boards)
    legal = np.zeros((m, 192), bool)
    for k in range(m):
        legal[k] = R.make_env(boards[k], hands[k]).obs()["action_mask"].astype(bool)
    for k in range(n_single):  # the illegal in-bounds anchors of a piece: the cell minus each of its offsets
        cr, cc = divmod(int(boards[k]).bit_length() - 1, 8)
        for s, p in enumerate(hands[k]):
            want = np.zeros((8, 8), bool)
            want[:O.BOARD - O.PIECE_H[p] + 1, :O.BOARD - O.PIECE_W[p] + 1] = True
            for dr, dc in O.PIECE_CELLS[p]:
                if 0 <= cr - dr and 0 <= cc - dc:
                    want[cr - dr, cc - dc] = False
            assert np.array_equal(legal[k, 64 * s:64 * s + 64].reshape(8, 8), want), labels[k]
    for k, (p, r, c) in enumerate(pairs(), start=n_single):  # exactly one anchor of p is legal: (r, c)
        assert np.nonzero(legal[k, 64:128])[0].tolist() == [r * 8 + c], labels[k]
    return {"n": m, "board": np.array(boards, np.uint64), "hand": _hand_words(hands, np.zeros((m, 3), bool)),
            "legal": legal, "labels": labels}


# ---------------------------------------------------------------------------------------------------------
# running the library on the atlas and comparing (shared by the host and the GPU test files)
# ---------------------------------------------------------------------------------------------------------
def expect(field, got, want, name_of, idx=None):
    """Exact equality of two arrays over positions; the failure names the first differing position."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (field, got.shape, want.shape)
    if got.size == 0:
        return
    bad = (got != want).reshape(len(got), -1)
    if bad.any():
        rows = np.nonzero(bad.any(axis=1))[0]
        j, k = int(rows[0]), int(np.nonzero(bad[rows[0]])[0][0])
        i = j if idx is None else int(idx[j])
        where = f"[{k}]" if bad.shape[1] > 1 else ""
        raise AssertionError(f"{field}{where} differs from the oracle at {name_of(i)}: got "
                             f"{got.reshape(bad.shape)[j, k]!r}, oracle {want.reshape(bad.shape)[j, k]!r} "
                             f"({len(rows)} of {len(bad)} positions differ)")


def packed_masks(mask_bool):
    """[..., 192] bool -> [..., 3] u64 in bbvec.h's mask layout (tests/_crowded.mask_bits per position)."""
    m = np.asarray(mask_bool, bool)
    return np.array([mask_bits(x) for x in m.reshape(-1, 192)], np.uint64).reshape(m.shape[:-1] + (3,))


def make_batch(device, autoreset, reward_config=None):
    """A DeviceEnvBatch on ``device`` that holds the atlas positions, each env seeded with its position's seed."""
    from runtime.device_env import DeviceEnvBatch

    pos = positions()
    batch = DeviceEnvBatch(pos["n"], seeds=[int(s) for s in pos["seed"]], reward_config=reward_config,
                           autoreset=autoreset, device=device)
    batch.set_state(**{k: pos[k] for k in ("board", "hand", "score", "combo", "max_combo", "moves", "lines", "blocks",
                                           "prev_holes", "prev_center")})
    return batch


def _expect_state(what, st, want, name_of):
    for k in STATE_FIELDS:
        expect(f"{what} state {k}", st[k], want[k], name_of)
    expect(f"{what} PCG64 state (high word)", st["rng"][:, 0], want["rng_hi"], name_of)
    expect(f"{what} PCG64 state (low word)", st["rng"][:, 1], want["rng_lo"], name_of)
    has = want["has32"]
    expect(f"{what} PCG64 buffered uint32", st["rng"][has, 2], want["uinteger"][has], name_of, np.nonzero(has)[0])


def check_step(device, custom=False):
    """bb_step of the crafted action of every position (no auto-reset): every output and the whole post-move state."""
    ref = reference(custom)
    pos, n = ref["pos"], ref["n"]
    name_of = functools.partial(describe, pos)
    batch = make_batch(device, autoreset=False, reward_config=CUSTOM_REWARDS if custom else None)
    mask = torch.zeros((n, 3), dtype=torch.int64, device=batch.device)
    batch.step(torch.from_numpy(pos["action"]).to(batch.device), want_info=True, want_f64=True, want_lines=True,
               mask_out=mask)
    batch.sync()
    expect("fp64 reward", batch.reward_f64.cpu().numpy(), ref["reward"], name_of)
    expect("f32 reward bits", batch.reward.cpu().numpy().view(np.uint32), ref["reward"].astype(np.float32).view(np.uint32),
           name_of)
    expect("terminated", batch.terminated.cpu().numpy().astype(bool), ref["term"], name_of)
    expect("lines", batch.lines.cpu().numpy().astype(np.int64), ref["move_lines"], name_of)
    info = batch.info_host()
    for k in INFO_FIELDS:
        expect(f"info {k}", info[k].astype(np.int64), ref["info"][k], name_of)
    ended = np.nonzero(ref["term"])[0]
    expect("info term_board", info["term_board"][ended], ref["post"]["board"][ended], name_of, ended)
    expect("info term_hand", info["term_hand"][ended], ref["post"]["hand"][ended], name_of, ended)
    _expect_state("post-move", batch.state(), ref["post"], name_of)
    expect("post-move mask", mask.cpu().numpy().view(np.uint64), packed_masks(ref["post_mask"]), name_of)
    batch.close()


def check_rollout(device):
    """bb_rollout with T = ROLLOUT_STEPS and auto-reset, the crafted action first: the recorded actions are the
    oracle's Philox policy's, and every step's reward bits, termination, lines and mask and the final state equal
    the oracle's replay."""
    ref, roll = reference(), rollout_reference()
    pos, n, T = ref["pos"], ref["n"], ROLLOUT_STEPS
    name_of = functools.partial(describe, pos)
    batch = make_batch(device, autoreset=True)
    dev = batch.device
    rew = torch.zeros((T, n), dtype=torch.float32, device=dev)
    term = torch.zeros((T, n), dtype=torch.uint8, device=dev)
    lines = torch.zeros((T, n), dtype=torch.uint8, device=dev)
    acts = torch.zeros((T, n), dtype=torch.int32, device=dev)
    masks = torch.zeros((T, n, 3), dtype=torch.int64, device=dev)
    nxt = torch.zeros(n, dtype=torch.int32, device=dev)
    batch.rollout(T, torch.from_numpy(pos["action"]).to(dev), rew, term, lines=lines, actions_out=acts, mask_out=masks,
                  next_action=nxt, policy_seed=POLICY_SEED, policy_step0=0)
    batch.sync()  # raises if the kernel reported a device-side failure
    want_masks = packed_masks(roll["mask"])
    for t in range(T):
        expect(f"rollout step {t} action", acts[t].cpu().numpy(), roll["action"][t], name_of)
        expect(f"rollout step {t} f32 reward bits", rew[t].cpu().numpy().view(np.uint32),
               roll["reward"][t].view(np.uint32), name_of)
        expect(f"rollout step {t} terminated", term[t].cpu().numpy().astype(bool), roll["term"][t], name_of)
        expect(f"rollout step {t} lines", lines[t].cpu().numpy().astype(np.int64), roll["lines"][t], name_of)
        expect(f"rollout step {t} mask", masks[t].cpu().numpy().view(np.uint64), want_masks[t], name_of)
    expect("rollout next_action", nxt.cpu().numpy(), roll["next_action"], name_of)
    _expect_state("rollout final", batch.state(), roll["final"], name_of)
    batch.close()


def position_tensors(cols, device, idx=None):
    """(board, hand, combo, prev) of the positions (all, or those at idx) as runtime.kernels takes them."""
    sel = slice(None) if idx is None else idx
    t = [torch.from_numpy(cols["board"][sel].view(np.int64).copy()), torch.from_numpy(cols["hand"][sel].view(np.int32).copy())]
    t += [torch.from_numpy(cols[k][sel].view(dt).copy()) if k in cols else None
          for k, dt in (("combo", np.int32), ("prev", np.int16))]
    return tuple(x.to(device) if x is not None else None for x in t)


def check_afterstates(out, idx=None):
    """An afterstates result ([len(idx), 192] tensors) against the oracle: all 192 legal bits, and the crafted
    action's board, score_gained, aux word and fp64 reward (left out where chance_end; their share is bounded)."""
    ref = reference()
    pos, one = ref["pos"], ref["one"]
    name_of = functools.partial(describe, pos)
    idx = np.arange(ref["n"]) if idx is None else np.asarray(idx)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    aux = got["aux"].view(np.uint32)
    expect("afterstates legal bits", (aux & 1).astype(bool), ref["legal"][idx], name_of, idx)
    rows, a = np.arange(len(idx)), pos["action"][idx]
    expect("afterstates board", got["board"].view(np.uint64)[rows, a], one["board"][idx], name_of, idx)
    expect("afterstates score_gained", got["score_gained"][rows, a].astype(np.int64), one["score"][idx], name_of, idx)
    for k, shift, width in (("dead", 1, 1), ("refill", 2, 1), ("lines", 8, 4), ("holes", 12, 7), ("centre", 19, 5),
                            ("mobility", 24, 8)):
        expect(f"afterstates aux {k}", ((aux[rows, a] >> shift) & ((1 << width) - 1)).astype(np.int64), one[k][idx],
               name_of, idx)
    want_aux = (1 | (one["dead"] << 1) | (one["refill"] << 2) | (one["lines"] << 8) | (one["holes"] << 12)
                | (one["centre"] << 19) | (one["mobility"] << 24)).astype(np.uint32)
    expect("afterstates aux word", aux[rows, a], want_aux[idx], name_of, idx)
    assert int(ref["chance_end"].sum()) * 100 <= ref["n"], f"{int(ref['chance_end'].sum())} chance_end positions"
    keep = ~ref["chance_end"][idx]
    expect("afterstates fp64 reward", got["reward"][rows, a][keep], one["reward"][idx][keep], name_of, idx[keep])


def check_greedy_and_plan(device, idx_of_subset=None):
    """bb_greedy_actions_pos and bb_plan_actions_pos (depth 3) on the one-piece-left subset (or the part of it at
    idx_of_subset): the oracle's arg-max, and a plan that is that one move."""
    from runtime import kernels as K

    pos, want = positions(), greedy_reference()
    sub = np.arange(len(greedy_subset())) if idx_of_subset is None else np.asarray(idx_of_subset)
    idx = greedy_subset()[sub]
    name_of = functools.partial(describe, pos)
    board, hand, combo, _ = position_tensors(pos, device, idx)
    for wname, w in GREEDY_WEIGHTS.items():
        action, value = K.greedy_actions(board, hand, w, combo=combo)
        expect(f"greedy action ({wname})", action.cpu().numpy(), want[wname][0][sub], name_of, idx)
        expect(f"greedy value ({wname})", value.cpu().numpy(), want[wname][1][sub], name_of, idx)
        res = K.plan_actions(board, hand, w, depth=3, combo=combo, want_plan=True)
        expect(f"plan action ({wname})", res["action"].cpu().numpy(), want[wname][0][sub], name_of, idx)
        expect(f"plan value ({wname})", res["value"].cpu().numpy(), want[wname][1][sub], name_of, idx)
        plan = res["plan"].cpu().numpy()
        expect(f"plan first ply ({wname})", plan[:, 0], want[wname][0][sub], name_of, idx)
        expect(f"plan later plies ({wname})", plan[:, 1:], np.full((len(idx), 2), -1, np.int32), name_of, idx)


def check_blockers(device):
    """The blocker boards through bb_obs (a handle that holds them) and through bb_afterstates_pos's legal bit."""
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    blk = blockers()
    m = blk["n"]
    name_of = lambda k: f"blocker board {k}: {blk['labels'][k]}"  # noqa: E731
    want = packed_masks(blk["legal"])
    batch = DeviceEnvBatch(m, seeds=list(range(m)), autoreset=False, device=device)
    batch.reset()
    batch.set_state(board=blk["board"], hand=blk["hand"])
    bits = torch.zeros((m, 3), dtype=torch.int64, device=batch.device)
    i8 = torch.zeros((m, 192), dtype=torch.int8, device=batch.device)
    batch.obs(mask_i8=i8, mask_bits=bits)
    batch.sync()
    expect("bb_obs mask bits", bits.cpu().numpy().view(np.uint64), want, name_of)
    expect("bb_obs int8 mask", i8.cpu().numpy().astype(bool), blk["legal"], name_of)
    batch.close()
    board, hand, _, _ = position_tensors(blk, batch.device)
    aux = K.afterstates(board, hand, out=K.afterstate_outputs(m, batch.device, want=("aux",)))["aux"]
    expect("bb_afterstates_pos legal bit", (aux.cpu().numpy().view(np.uint32) & 1).astype(bool), blk["legal"], name_of)
