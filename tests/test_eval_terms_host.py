"""The shape terms and the search with them on the host backend (bb_board_terms / bb_plan_actions_ext of
libbbvec_host.so) and their Python surface, on the CPU, no GPU involved.

The references are tests/_eval_terms_ref.py's: the four terms restated cell by cell, and tests/_plan_ref.py's
level-by-level search with the terms added to every leaf.  Zero shape weights are held to the existing
``plan_actions_each``, so the new entry point cannot pass by agreeing only with itself.
"""
import json

import numpy as np
import pytest
import torch

import _afterstates_ref as R
import _eval_terms_ref as E

KEYS = ("action", "value", "plan", "leaves")
CPU = torch.device("cpu")
NAMES = list(E.SETS)


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


@pytest.fixture(scope="module")
def ref(host):
    return R.reference()


def _i64(boards):
    return torch.from_numpy(np.asarray(boards, np.uint64).view(np.int64).copy())


def _ext(cols, rows, depth):
    from runtime import kernels as K

    return K.plan_actions_ext(cols[0], cols[1], rows, depth, combo=cols[2], want_plan=True, want_leaves=True)


def _assert_same(got, want, what):
    for k in KEYS:
        g, x = torch.as_tensor(got[k]), torch.as_tensor(want[k])
        bad = torch.nonzero((g != x).reshape(g.shape[0], -1).any(dim=1)).flatten()[:4]
        assert bad.numel() == 0, (what, k, bad.tolist(), g[bad].tolist(), x[bad].tolist())


# ---------------------------------------------------------------------------------------------------------------
# the terms
# ---------------------------------------------------------------------------------------------------------------
def test_terms_equal_the_cell_reference(host):
    from runtime import kernels as K

    boards, want, where = E.reference_terms()
    got = K.board_terms(_i64(boards)).numpy()
    assert got.dtype == np.int32 and got.shape == (len(boards), 4)
    for fam, sl in where.items():
        bad = np.nonzero((got[sl] != want[sl]).any(axis=1))[0][:4]
        assert bad.size == 0, (fam, [hex(int(b)) for b in boards[sl][bad]], got[sl][bad], want[sl][bad])
    # the pinned values of the issue, and what the families are for
    assert got[where["basic"]].tolist() == [[32, 36, 64, 37], [0, 0, 0, 0], [128, 0, 0, 5]]
    w3, w15, w51 = (got[where[k]] for k in ("window3x3", "window1x5", "window5x1"))
    assert (w3[:, 1] == 1).all() and (w3[:, 2] == 0).all() and (w3[:, 3] == 33).all() and (w3[:, 0] == 12).all()
    for w in (w15, w51):
        assert (w[:, 1] == 0).all() and (w[:, 2] == 1).all() and (w[:, 0] == 12).all()
    assert sorted(set(w15[:, 3].tolist())) == sorted(set(w51[:, 3].tolist())) == [5]  # single, domino, trio, two bars
    # one anchor each: the window's own
    from game.pieces import PIECE_LIST

    assert [p.name for p in (PIECE_LIST[36], PIECE_LIST[15], PIECE_LIST[16])] == ["SQUARE_3x3", "I5_H", "I5_V"]
    rnd = got[where["random"]]
    assert rnd[:, 3].min() == 0 and rnd[:, 3].max() == 37 and len(set(rnd[:, 3].tolist())) > 20
    assert rnd[:, 1].max() == 36 and rnd[:, 2].max() == 64 and rnd[:, 0].max() > 80


def test_term_identities_the_reference_confirms(host):
    """Asserted on the library's answers only because the cell-by-cell reference shows them on the whole set."""
    from runtime import kernels as K

    boards, want, _ = E.reference_terms()
    holes = np.array([R.O.count_holes(np.array([[(int(b) >> (r * 8 + c)) & 1 for c in range(8)] for r in range(8)]))
                      for b in boards[::7]])
    filled = np.array([bin(int(b)).count("1") for b in boards])
    for t in (want, K.board_terms(_i64(boards)).numpy().astype(np.int64)):
        assert (t[::7, 0] >= 4 * holes).all()                      # a hole is closed on all four sides
        assert ((t[:, 3] == 0) == (filled == 64)).all()            # nothing fits exactly on the full board
        assert (t[:, 1] <= 36).all() and (t[:, 2] <= 64).all() and (t[:, 0] <= 128).all()
        assert ((t[:, 1] > 0) <= (t[:, 3] >= 33)).all()            # where the square fits, every 3x3-box piece does


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_terms_sizes_and_the_handle_form(host, n):
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    boards = E.random_boards(n, 5 + n) if n else np.zeros(0, np.uint64)
    buf = torch.full((n * 4 + 4,), -99, dtype=torch.int32)
    got = K.board_terms(_i64(boards), out=buf[:n * 4].view(n, 4))
    assert np.array_equal(got.numpy(), E.cell_terms(boards)) and (buf[n * 4:] == -99).all()
    if n:
        env = DeviceEnvBatch(n, list(range(n)), autoreset=False, device="cpu")
        env.reset()
        env.set_state(board=boards)
        assert torch.equal(env.board_terms(), got)
        env.close()


# ---------------------------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_ext_equals_the_reference_search(ref, depth):
    from runtime import kernels as K

    idx, want = E.reference_plans(depth, depth < 3)  # depth 3: the trees of at most 20,000 leaves
    assert len(idx) == ref["n"] if depth < 3 else 40 <= len(idx) < ref["n"]
    cols = R.tensors(ref, CPU, idx)[:3]
    for name, w in E.SETS.items():
        _assert_same(_ext(cols, K.eval_rows(w), depth), want[name], f"{name} depth {depth}")
    changed = {k: E.plans_changed(want, k) for k in NAMES if k != "zero4"}
    assert all(v >= 5 for v in changed.values()), changed  # every set moves plans at every depth


@pytest.mark.slow
def test_ext_equals_the_reference_search_on_the_whole_set_at_depth_3(ref):
    from runtime import kernels as K

    idx, want = E.reference_plans(3, True)  # asserts the issue's plan-change counts itself
    cols = R.tensors(ref, CPU)[:3]
    for name, w in E.SETS.items():
        _assert_same(_ext(cols, K.eval_rows(w), 3), want[name], f"{name} depth 3, whole set")


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_zero_shape_weights_equal_plan_actions_each(ref, depth):
    from _weights_each import SETS as BASES
    from runtime import kernels as K

    n = ref["n"]
    cols = R.tensors(ref, CPU)[:3]
    for base in BASES + [E.SETS["zero4"]]:
        want = K.plan_actions_each(cols[0], cols[1], K.weight_rows(base, n=n), depth, combo=cols[2], want_plan=True,
                                   want_leaves=True)
        _assert_same(_ext(cols, K.eval_rows(base), depth), want, f"shared row, depth {depth}")
        _assert_same(_ext(cols, K.eval_rows(base, n=n), depth), want, f"own rows, depth {depth}")


def test_stride_0_equals_replicated_rows_and_interleaved_rows_equal_per_set_calls(ref):
    from runtime import kernels as K
    from runtime.device_env import DeviceEnvBatch

    n = ref["n"]
    cols = R.tensors(ref, CPU)[:3]
    per_set = [_ext(cols, K.eval_rows(E.SETS[k]), 2) for k in NAMES]
    for k, shared in zip(NAMES, per_set):
        _assert_same(_ext(cols, K.eval_rows(E.SETS[k], n=n), 2), shared, f"replicated {k}")
    which = (np.arange(n) + 3) % len(NAMES)
    rows = K.eval_rows([E.SETS[NAMES[j]] for j in which])
    want = {k: torch.stack([r[k] for r in per_set])[torch.as_tensor(which), torch.arange(n)] for k in KEYS}
    got = _ext(cols, rows, 2)
    _assert_same(got, want, "interleaved rows")
    assert any(not torch.equal(per_set[0]["action"], r["action"]) for r in per_set[1:])

    env = DeviceEnvBatch(n, list(range(n)), autoreset=False, device="cpu")
    env.reset()
    R.set_positions(env, ref["envs"])
    before = env.state()
    o = {"action": torch.full((n,), -7, dtype=torch.int32), "value": torch.full((n,), 5, dtype=torch.int64),
         "plan": torch.full((n, 3), -7, dtype=torch.int32), "leaves": torch.full((n,), -7, dtype=torch.int32)}
    env.plan_actions_ext(o["action"], rows, 2, value=o["value"], plan=o["plan"], leaves=o["leaves"])
    _assert_same(o, want, "handle form, own rows")
    env.plan_actions_ext(o["action"], K.eval_rows(E.SETS["all"]), 2, value=o["value"], plan=o["plan"],
                         leaves=o["leaves"])
    _assert_same(o, per_set[NAMES.index("all")], "handle form, shared row")
    after = env.state()
    assert all(np.array_equal(before[k], after[k]) for k in before), "the handle form changed the state"
    env.close()


def test_no_legal_action_and_bad_rows(ref):
    from _weights_each import no_action_positions
    from runtime import kernels as K
    from runtime.lib import BBNativeError

    board, hand = no_action_positions(ref)
    rows = K.eval_rows([E.SETS[NAMES[i % len(NAMES)]] for i in range(8)])
    for depth in (1, 2, 3):
        for r in (rows, K.eval_rows(E.SETS["mixed"])):
            got = K.plan_actions_ext(board, hand, r, depth, want_plan=True, want_leaves=True)
            assert (got["action"] == 0).all() and (got["value"] == R.INT64_MIN).all()
            assert (got["plan"] == -1).all() and (got["leaves"] == 0).all()
    good = K.eval_rows({}, n=8)
    bad = {"dtype": good.long(), "rows": K.eval_rows({}, n=3), "width": torch.zeros((8, 8), dtype=torch.int32),
           "contiguity": torch.zeros((8, 24), dtype=torch.int32)[:, ::2], "not a tensor": [[0] * 12] * 8}
    for what, r in bad.items():
        with pytest.raises(BBNativeError, match=r"rows must be a contiguous torch.int32 \[1, 12\] or \[8, 12\]"):
            K.plan_actions_ext(board, hand, r, 2)
    with pytest.raises(BBNativeError, match="depth must be 1..3"):
        K.plan_actions_ext(board, hand, good, 4)


# ---------------------------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------------------------
def test_eval_rows_and_the_refusals_of_the_eight_weight_forms(host):
    import ctypes as C

    from agents.greedy import GreedyAgent, HandPlanAgent, PopulationPlanAgent, TwoHandPlanAgent
    from runtime import kernels as K
    from runtime import lib as L

    assert L.EVAL_FIELDS == L.GREEDY_FIELDS + ("perimeter", "room3", "room5", "fits") and L.TERM_FIELDS == L.EVAL_FIELDS[8:]
    w = {k: 10 + j for j, k in enumerate(L.EVAL_FIELDS)}
    one = K.eval_rows(w)
    assert one.dtype == torch.int32 and one.is_contiguous() and one.tolist() == [list(range(10, 22))]
    assert list((C.c_int32 * 12).from_buffer_copy(bytes(L.eval_weights(w)))) == one[0].tolist()
    assert C.sizeof(L.EvalWeights) == 48
    assert K.eval_rows({"room5": -3}, n=3).tolist() == [[0] * 10 + [-3, 0]] * 3
    assert K.eval_rows([{"fits": E.BIG}, {"lines": -E.BIG}]).tolist() == [[0] * 11 + [E.BIG], [-E.BIG] + [0] * 11]
    for bad in ({"room4": 1}, [{}, {"perimetre": 1}]):
        with pytest.raises(ValueError, match="unknown evaluation weights"):
            K.eval_rows(bad)
    with pytest.raises(ValueError):
        K.eval_rows([{}, {}], n=3)
    # the eight-weight forms refuse the new names as they refuse any unknown name
    with pytest.raises(ValueError, match="unknown greedy weights"):
        K.weight_rows({"room3": 1})
    with pytest.raises(ValueError, match="unknown greedy weights"):
        L.greedy_weights({"fits": 1})
    for cls in (GreedyAgent, TwoHandPlanAgent):
        with pytest.raises(ValueError, match="no extended kernel yet"):
            cls({"perimeter": -3}, device="cpu")
        with pytest.raises(ValueError, match="unknown greedy weights"):
            cls({"linez": 1}, device="cpu")
    assert HandPlanAgent({"fits": 2}, device="cpu").weights["fits"] == 2
    with pytest.raises(ValueError, match="unknown evaluation weights"):
        HandPlanAgent({"room4": 2}, device="cpu")
    with pytest.raises(ValueError, match="depth 1..3"):
        PopulationPlanAgent(K.eval_rows({}, n=2), depth=0, device="cpu")


def _play(agent, seeds, moves):
    """The actions an agent plays on a host env batch, [moves, N], and the positions it met."""
    from runtime.device_env import DeviceEnvBatch

    env = DeviceEnvBatch(len(seeds), list(seeds), autoreset=False, device="cpu")
    env.reset()
    out = torch.zeros(len(seeds), dtype=torch.int32)
    acts, met = [], []
    for _ in range(moves):
        st = env.state()
        met.append((st["board"].copy(), st["hand"].copy(), st["combo"].copy()))
        agent.act_env(env, out)
        acts.append(out.clone())
        env.step(out)
    env.close()
    return torch.stack(acts), met


def test_hand_plan_agent_with_shape_weights_plays_the_reference_search(host, tmp_path):
    from agents.greedy import DEFAULT_WEIGHTS, HandPlanAgent

    agent = HandPlanAgent(E.SETS["all"], depth=2, device="cpu")
    acts, met = _play(agent, [50, 51, 52, 53], 20)
    for t, (board, hand, combo) in enumerate(met):
        want = E.chained_ext(board, hand, combo, 2, {"all": E.SETS["all"]})["all"]["action"]
        assert acts[t].tolist() == want.tolist(), t
    plain, _ = _play(HandPlanAgent(depth=2, device="cpu"), [50, 51, 52, 53], 20)
    assert not torch.equal(acts, plain)
    # the four at 0: today's path, today's moves
    zeros, _ = _play(HandPlanAgent({k: 0 for k in E.TERMS}, depth=2, device="cpu"), [50, 51, 52, 53], 20)
    assert torch.equal(zeros, plain)
    # save / load carry the new names; select_action takes the same path
    path = str(tmp_path / "w.json")
    agent.save(path)
    assert json.load(open(path))["weights"]["room5"] == 2
    again = HandPlanAgent(device="cpu")
    again.load(path)
    assert again.weights == {**DEFAULT_WEIGHTS, **E.SETS["all"]} and again.depth == 2
    reacts, _ = _play(again, [50, 51, 52, 53], 6)
    assert torch.equal(reacts, acts[:6])


def test_evaluate_population_with_twelve_wide_dicts_equals_per_agent_evaluation(host):
    from agents.greedy import HandPlanAgent
    from evaluation.evaluate import evaluate_agent
    from evaluation.tune import evaluate_population

    sets = [E.SETS[k] for k in ("zero4", "r3", "all", "mixed")]
    got = evaluate_population(sets, 3, 25, 9, depth=2, device="cpu")
    for c, w in enumerate(sets):
        one = evaluate_agent(HandPlanAgent(w, depth=2, device="cpu"), num_episodes=3, seed=9, max_moves=25)
        assert got[c].tolist() == [int(s) for s in one["scores"]], c
    assert not torch.equal(got[0], got[2])


def _records(path):
    recs = [json.loads(line) for line in open(path)]
    for r in recs:
        r.pop("wall_s", None)
    return recs


def test_tune_terms(host, tmp_path):
    from evaluation.tune import tune

    kw = dict(agent="plan", depth=2, population=6, games=2, moves=15, generations=2, seed=3, holdout_games=2,
              device="cpu")
    a = tune(log=str(tmp_path / "a.jsonl"), **kw)
    b = tune(log=str(tmp_path / "b.jsonl"), terms=(), **kw)
    assert _records(tmp_path / "a.jsonl") == _records(tmp_path / "b.jsonl")  # no terms: what it is without the argument
    assert set(a["weights"]) == set(R.DEFAULT_WEIGHTS) and "terms" not in a["settings"] and a["weights"] == b["weights"]
    c = tune(log=str(tmp_path / "c.jsonl"), output=str(tmp_path / "c.json"), terms=("room3",), **kw)
    d = tune(log=str(tmp_path / "d.jsonl"), terms=("room3",), **kw)
    assert _records(tmp_path / "c.jsonl") == _records(tmp_path / "d.jsonl")  # deterministic for a seed
    assert "room3" in c["weights"] and set(c["weights"]) == set(R.DEFAULT_WEIGHTS) | {"room3"}
    assert c["settings"]["terms"] == ["room3"] and c["init"]["room3"] == 0
    gen0 = _records(tmp_path / "c.jsonl")[0]
    assert gen0["mean_played"]["room3"] == 0 and len(gen0["mean"]) == 9  # the term starts at 0
    from agents.greedy import HandPlanAgent

    agent = HandPlanAgent(device="cpu")
    agent.load(str(tmp_path / "c.json"))
    assert agent.weights["room3"] == c["weights"]["room3"]
    with pytest.raises(ValueError, match="terms must be"):
        tune(terms=("room4",), **kw)
    with pytest.raises(ValueError, match="agent 'plan'"):
        tune(terms=("room3",), **{**kw, "agent": "greedy"})
