"""The search waves' straight-line quick pass and the exact phase without its two known-failed first leaves
(csrc/bb_solver.h: pair_quick_bf, gen_hands_quota, gen_hands_multi, gen_hand_wave, slow_phase_wave), bit for
bit against the oracles on the boards where the exact phase decides hands.

What the rewrite could lose, and where it is pinned:

* the exact phase no longer tests the first leaf of each order (the quick test has), so an undecided slot whose
  only successful leaves are later ones must still be found, and a slot whose lists become empty must give "no
  success" without stalling the scan;
* the exact trip and the quick pass read their table rows for every lane and gate the result, so lanes past
  the last task or slot must not count;
* an attempt with more than 64 exact tasks runs a scan of several trips.

The starts are crowded boards (tests/_crowded.py) at fills 0.8, 0.95, -1.0 and -2.0, 128 of each.  Whether
they hold those cases is computed here on the CPU from the start states, with a bitboard replay of the first
step's hand generation in Python ints (anchors, clear, the quick test, both leaf orders), and asserted as
floors.  Only slots the device cannot skip are counted: those of failed attempts before the accepted one, and
those of an accepted attempt in which no slot quick-accepts.  Checked on a CPU-only machine for the seeds
below, Test B's 512 starts / Test A's 300 (40 + 40 + 110 + 110 of the four fills, their streams after a
reset): undecided slots with a successful later leaf in attempts that nothing else decides 31 / 25 (floor 20);
needed slots with |A2| = 1, A3 = 0 96 / 63 and the mirror 99 / 53 (floor 1 each); the largest exact task count
of one attempt after its first four slots and without the first leaves 362 / 362 (floor 65); envs with more
than one attempt 346 of 512 / 231 of 300 (floor a third); envs at 100 attempts 5 / 4 (floor 1).  The replay's
attempt counts are checked against oracle.bb_game's attempts_last in Test B.

The GPU shapes are the smallest that reach those paths: 300 envs are two workgroups of the rollout kernel (256
+ 44: one full and one partly live env wave), three launches of 12 steps carry hand and stream across launch
boundaries; 512 envs of one bb_step put several parked envs into every search call of the step kernels.
"""
import numpy as np
import pytest
import torch

from _crowded import crowded_setup
from oracle import bb_game as O
from oracle import c_oracle as CO

SEED = 0xB10C
FILLS = (0.8, 0.95, -1.0, -2.0)
PER_FILL = 128
SEED_BASE = 7300
N_STEP = PER_FILL * len(FILLS)  # Test B
PER_FILL_A = (40, 40, 110, 110)  # Test A: the holes-only boards carry most of the later-leaf decisions
N, T, LAUNCHES = sum(PER_FILL_A), 12, 3

# --------------------------------------------------------------------------
# Bitboard replay of _generate_new_pieces (engine.py:155-172) in Python ints
# --------------------------------------------------------------------------
_M64 = (1 << 64) - 1
_SHAPE = [sum(1 << (r * 8 + c) for r, c in cells) for cells in O.PIECE_CELLS]
_OFFS = [[r * 8 + c for r, c in cells] for cells in O.PIECE_CELLS]
_LEGAL = [sum(1 << (r * 8 + c) for r in range(8 - O.PIECE_H[p] + 1) for c in range(8 - O.PIECE_W[p] + 1))
          for p in range(O.NUM_PIECES)]
_ND = [[len({a - b for a in _OFFS[y] for b in _OFFS[z]}) for z in range(O.NUM_PIECES)] for y in range(O.NUM_PIECES)]
_ROWS = [0xFF << (8 * r) for r in range(8)]
_COLS = [0x0101010101010101 << c for c in range(8)]


def _anchors(p, B):
    blocked = 0
    for o in _OFFS[p]:
        blocked |= B >> o
    return _LEGAL[p] & ~blocked & _M64


def _clear(B):
    full = 0
    for m in _ROWS + _COLS:
        if B & m == m:
            full |= m
    return B & ~full


def _bits(x):
    while x:
        b = x & -x
        yield b.bit_length() - 1
        x ^= b


def _later_leaf(B1, b, c, A2, A3):
    """Some leaf after the first of either order succeeds (the exact phase's task lists A & (A - 1))."""
    for q in _bits(A2 & (A2 - 1)):
        if _anchors(c, _clear(B1 | (_SHAPE[b] << q))):
            return True
    for r in _bits(A3 & (A3 - 1)):
        if _anchors(b, _clear(B1 | (_SHAPE[c] << r))):
            return True
    return False


def _attempt(B, hand):
    """Every level-1 slot of one attempt, f-major: (q, later, tasks, kind) with q the quick verdict (0 reject,
    1 accept, 2 undecided: both first leaves failed), later = a later leaf succeeds, tasks = the exact tasks left
    after the first leaves, kind = 'b' for |A2| = 1, A3 = 0, 'c' for the mirror (both lists become empty)."""
    out = []
    for f in range(3):
        b, c = hand[1 if f == 0 else 0], hand[1 if f == 2 else 2]
        for p in _bits(_anchors(hand[f], B)):
            B1 = _clear(B | (_SHAPE[hand[f]] << p))
            A2, A3 = _anchors(b, B1), _anchors(c, B1)
            n2, n3 = bin(A2).count("1"), bin(A3).count("1")
            if not (A2 | A3):
                out.append((0, False, 0, None))
                continue
            acc = (A2 and n3 > _ND[b][c]) or (A3 and n2 > _ND[b][c])
            if not acc and A2:
                acc = _anchors(c, _clear(B1 | (_SHAPE[b] << ((A2 & -A2).bit_length() - 1)))) != 0
            if not acc and A3:
                acc = _anchors(b, _clear(B1 | (_SHAPE[c] << ((A3 & -A3).bit_length() - 1)))) != 0
            if acc:
                out.append((1, False, 0, None))
                continue
            kind = "b" if (n2 == 1 and n3 == 0) else ("c" if (n3 == 1 and n2 == 0) else None)
            out.append((2, _later_leaf(B1, b, c, A2, A3), max(n2 - 1, 0) + max(n3 - 1, 0), kind))
    return out


def _coverage(boards, acts, rngs):
    """Replay the first step's hand generation of every env.  Only slots the device has to decide count: those of
    failed attempts before the accepted one, and those of an accepted attempt in which no slot quick-accepts."""
    cov = dict(later_only=0, empty_b=0, empty_c=0, max_tasks=0, attempts=[])
    for B0, a, rng in zip(boards, acts, rngs):
        B = _clear(int(B0) | (1 << (int(a) & 63)))  # SINGLE on the action's cell
        att = 0
        for att in range(1, O.Engine.MAX_ATTEMPTS + 1):
            slots = _attempt(B, O.draw_hand(rng))
            quick = any(s[0] == 1 for s in slots)
            won = quick or any(s[1] for s in slots)
            if not quick:
                und = [s for s in slots if s[0] == 2]
                cov["empty_b"] += sum(s[3] == "b" for s in und)
                cov["empty_c"] += sum(s[3] == "c" for s in und)
                # past the first pass's quota of four slots, so the tasks share passes of up to 64 slots
                cov["max_tasks"] = max(cov["max_tasks"], sum(s[2] for s in slots[4:] if s[0] == 2))
                if won:
                    cov["later_only"] += sum(s[1] for s in und)
            if won:
                break
        cov["attempts"].append(att)
    cov["attempts"] = np.array(cov["attempts"])
    return cov


def _assert_floors(cov, n):
    print({k: (v if k != "attempts" else (int((v > 1).sum()), int((v == 100).sum()))) for k, v in cov.items()})
    assert cov["later_only"] >= 20
    assert cov["empty_b"] >= 1 and cov["empty_c"] >= 1
    assert cov["max_tasks"] > 64
    assert (cov["attempts"] > 1).sum() * 3 >= n and (cov["attempts"] == 100).any()


# --------------------------------------------------------------------------
# The starts, shared by both tests
# --------------------------------------------------------------------------
_START = {}
_REF = {}


def _start():
    """512 crowded starts, 128 per fill; env i of fill group g has seed SEED_BASE + 128 g + i."""
    if not _START:
        parts = [crowded_setup(fill, PER_FILL, seed_base=SEED_BASE + PER_FILL * g) for g, fill in enumerate(FILLS)]
        _START["board"] = np.concatenate([p[0]["board"] for p in parts])
        _START["hand"] = np.concatenate([p[0]["hand"] for p in parts])
        _START["acts"] = np.concatenate([p[1] for p in parts])
        _START["refs"] = [e for p in parts for e in p[2]]
        _START["seeds"] = np.arange(SEED_BASE, SEED_BASE + N_STEP, dtype=np.uint64)
    return _START


def _rollout_pick():
    """Test A's 300 starts: the first PER_FILL_A[g] of fill group g."""
    return np.concatenate([np.arange(k) + PER_FILL * g for g, k in enumerate(PER_FILL_A)])


# --------------------------------------------------------------------------
# Test A: rollout parity on the crowded starts
# --------------------------------------------------------------------------
def _oracle_env():
    s, pick = _start(), _rollout_pick()
    c = CO.CVecEnv(s["seeds"][pick])
    c.reset()
    c.set_board_hand(board=s["board"][pick], hand=s["hand"][pick])
    return c


def _oracle():
    """The C oracle's three launches, computed once, and the coverage of its starts."""
    if "ref" not in _REF:
        s, pick = _start(), _rollout_pick()
        c = _oracle_env()
        st = c.state()
        rngs = []
        for i, seed in enumerate(s["seeds"][pick]):  # env i's stream after the reset's draws
            g = np.random.default_rng(int(seed))
            d = g.bit_generator.state
            d["state"]["state"] = (int(st["rng"][i, 0]) << 64) | int(st["rng"][i, 1])
            d["has_uint32"] = int((int(st["hand"][i]) >> 22) & 1)
            d["uinteger"] = int(st["rng"][i, 2])
            g.bit_generator.state = d
            rngs.append(g)
        _REF["cov"] = _coverage(s["board"][pick], s["acts"][pick], rngs)
        outs, a = [], s["acts"][pick]
        for k in range(LAUNCHES):
            outs.append(c.rollout(T, a, policy_seed=SEED, policy_step0=k * T))
            a = outs[-1]["next_action"]
        ref = {key: np.concatenate([o[key] for o in outs]) for key in ("reward", "terminated", "lines", "actions",
                                                                        "mask")}
        ref["next_action"] = a
        _REF["ref"] = (ref, c.state())
        c.close()
    return _REF["ref"], _REF["cov"]


def _gpu_env(cuda):
    from runtime.device_env import DeviceEnvBatch

    s, pick = _start(), _rollout_pick()
    env = DeviceEnvBatch(N, seeds=[int(x) for x in s["seeds"][pick]], device=cuda)
    env.reset()
    has32 = env.state()["hand"] & np.uint32(1 << 22)  # the stream's buffered half survives the new hand
    env.set_state(board=s["board"][pick], hand=s["hand"][pick] | has32)
    return env, torch.tensor(s["acts"][pick], dtype=torch.int32, device=cuda)


def _finish(env, out, a, cuda):
    env.sync()
    mb = torch.zeros((N, 3), dtype=torch.int64, device=cuda)
    env.obs(mask_bits=mb)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["mask"] = out["mask"].view(np.uint64)
    out["next_action"] = a.cpu().numpy()
    st = env.state()
    st["mask"] = mb.cpu().numpy().view(np.uint64)
    env.close()
    return out, st


def _gpu_rollout(cuda):
    env, a = _gpu_env(cuda)
    nxt = torch.zeros_like(a)
    steps = T * LAUNCHES
    out = {"reward": torch.zeros((steps, N), dtype=torch.float32, device=cuda),
           "terminated": torch.zeros((steps, N), dtype=torch.uint8, device=cuda),
           "lines": torch.zeros((steps, N), dtype=torch.uint8, device=cuda),
           "actions": torch.zeros((steps, N), dtype=torch.int32, device=cuda),
           "mask": torch.zeros((steps, N, 3), dtype=torch.int64, device=cuda)}
    for k in range(LAUNCHES):
        lo, hi = k * T, (k + 1) * T
        env.rollout(T, a, out["reward"][lo:hi], out["terminated"][lo:hi], lines=out["lines"][lo:hi],
                    actions_out=out["actions"][lo:hi], mask_out=out["mask"][lo:hi], next_action=nxt,
                    policy_seed=SEED, policy_step0=lo)
        a, nxt = nxt, a
        env.sync()  # raises if a wave left through an iteration cap
    return _finish(env, out, a, cuda)


def _gpu_chained(cuda):
    env, a = _gpu_env(cuda)
    nxt = torch.zeros_like(a)
    mb = torch.zeros((N, 3), dtype=torch.int64, device=cuda)
    rew, term, lines, acts, masks = [], [], [], [], []
    for t in range(T * LAUNCHES):
        acts.append(a.clone())
        env.step(a, next_action=nxt, want_lines=True, policy_seed=SEED, policy_step=t + 1, mask_out=mb)
        rew.append(env.reward.clone())
        term.append(env.terminated.clone())
        lines.append(env.lines.clone())
        masks.append(mb.clone())
        a, nxt = nxt, a
    out = {"reward": torch.stack(rew), "terminated": torch.stack(term), "lines": torch.stack(lines),
           "actions": torch.stack(acts), "mask": torch.stack(masks)}
    return _finish(env, out, a, cuda)


def _assert_same(ref, got, what):
    (ro, rs), (go, gs) = ref, got
    for k in ("reward", "terminated", "lines", "actions", "mask", "next_action"):
        a, b = (ro[k].view(np.uint32), go[k].view(np.uint32)) if k == "reward" else (ro[k], go[k])
        assert np.array_equal(a, b), f"{what}: {k}"
    for k in ("board", "hand", "score", "combo", "max_combo", "moves", "lines", "blocks", "prev_holes",
              "prev_center", "mask"):
        assert np.array_equal(rs[k], gs[k]), f"{what}: state {k}"
    assert np.array_equal(rs["rng"][:, :2], gs["rng"][:, :2]), f"{what}: pcg state"
    has = ((rs["hand"] >> np.uint32(22)) & np.uint32(1)).astype(bool)  # `uinteger` counts only while buffered
    assert np.array_equal(rs["rng"][has, 2], gs["rng"][has, 2]), f"{what}: pcg uinteger"


def test_starts_hold_the_exact_phase_cases():
    """The floors of the module docstring, on the starts of both tests (CPU only)."""
    s = _start()
    rngs = [np.random.default_rng(int(x)) for x in s["seeds"]]
    _assert_floors(_coverage(s["board"], s["acts"], rngs), N_STEP)
    _assert_floors(_oracle()[1], N)


@pytest.mark.gpu
def test_rollout_on_exact_phase_boards(cuda):
    """bb_rollout, three launches of 12 steps from 300 of the starts, against the C oracle and against 36 chained
    bb_step calls: reward bits, terminated, lines, actions, the 192-bit masks, the next action and the final
    state with the PCG64 state."""
    ref, cov = _oracle()
    _assert_floors(cov, N)
    got = _gpu_rollout(cuda)
    _assert_same(ref, got, "rollout vs C oracle")
    _assert_same(_gpu_chained(cuda), got, "rollout vs chained steps")


# --------------------------------------------------------------------------
# Test B: one bb_step on all 512 starts, every step-kernel path
# --------------------------------------------------------------------------
def _step_reference():
    """oracle.bb_game.Env's step of every start, computed once: reward, termination, hand, stream, attempts."""
    if "step" not in _REF:
        s = _start()
        rows = []
        for env, a in zip(s["refs"], s["acts"]):
            _, r, t, _, inf = env.step(int(a))
            st = env.engine.rng.bit_generator.state
            rows.append(dict(reward=r, term=t, score=inf["score"], hand=list(env.engine.hand),
                             state=st["state"]["state"], has=bool(st["has_uint32"]), uinteger=st["uinteger"],
                             attempts=env.engine.attempts_last))
        rngs = [np.random.default_rng(int(x)) for x in s["seeds"]]
        cov = _coverage(s["board"], s["acts"], rngs)
        assert np.array_equal(cov["attempts"], [r["attempts"] for r in rows])  # the replay is the engine's loop
        _REF["step"] = (rows, cov)
    return _REF["step"]


@pytest.mark.gpu
@pytest.mark.parametrize("pack,kernels", [("8,32", "1"), ("1,0", "1"), ("8,32", "2"), ("1,0", "2")])
def test_step_on_exact_phase_boards(cuda, pack, kernels, monkeypatch):
    """One bb_step on the 512 starts under both pack schedules, fused (1) and as step + escalate kernels (2):
    hand, stream, reward and termination against oracle.bb_game.Env."""
    from runtime.device_env import DeviceEnvBatch

    rows, cov = _step_reference()
    _assert_floors(cov, N_STEP)
    first, nxt = pack.split(",")
    monkeypatch.setenv("BB_PACK_FIRST", first)
    monkeypatch.setenv("BB_PACK_NEXT", nxt)
    monkeypatch.setenv("BB_STEP_KERNELS", kernels)
    s = _start()
    dev = DeviceEnvBatch(N_STEP, seeds=[int(x) for x in s["seeds"]], device=cuda)
    dev.set_state(board=s["board"], hand=s["hand"], prev_holes=np.zeros(N_STEP), prev_center=np.zeros(N_STEP))
    dev.step(torch.from_numpy(s["acts"]).to(cuda), want_f64=True, want_info=True)
    st = dev.state()
    rew = dev.reward_f64.cpu().numpy()
    term = dev.terminated.cpu().numpy()
    info = dev.info_host()
    for i, r in enumerate(rows):
        assert rew[i] == r["reward"], i
        assert bool(term[i]) == r["term"], i
        assert info[i]["score"] == r["score"], i
        if r["term"]:  # auto-reset happened; the terminal hand is in info
            h = int(info[i]["term_hand"])
            assert [(h >> (6 * k)) & 63 for k in range(3)] == r["hand"], i
            continue
        h = int(st["hand"][i])
        assert [(h >> (6 * k)) & 63 for k in range(3)] == r["hand"], i
        assert (int(st["rng"][i, 0]) << 64 | int(st["rng"][i, 1])) == r["state"], i
        assert bool((h >> 22) & 1) == r["has"], i
        if r["has"]:
            assert int(st["rng"][i, 2]) == r["uinteger"], i
    dev.close()
