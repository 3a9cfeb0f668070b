"""``PopulationTwoHandAgent`` on the host backend (CPU): with equal rows it plays move for move what the existing
two-hand agents play (they are its reference and stay as they are), and with rows of its own every env plays as its own
single-set agent."""
import pytest
import torch

import _plan2_ref as P2
from _plan2_ref import play, population


@pytest.fixture(scope="module")
def host():
    from runtime import lib as L
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    return L.load_host()


@pytest.mark.parametrize("depth,games,moves", [(2, 4, 12), (3, 2, 3)])
def test_equal_rows_play_the_existing_two_hand_agents(host, depth, games, moves):
    from agents.greedy import TwoHandPlanAgent, TwoHandShapeAgent, two_hand_agent_class

    seeds = [3, 5, 8, 13][:games]
    kw = dict(depth=depth, candidates=3, deals=2, seed=9)
    for w, cls in ((P2.SHAPED, TwoHandShapeAgent), (P2.R.DEFAULT_WEIGHTS, TwoHandPlanAgent)):
        assert two_hand_agent_class(w) is cls
        want = play(cls(w, device="cpu", **kw), seeds, moves)
        agent = population(w, games, **kw)
        assert play(agent, seeds, moves) == want and agent.moves == moves
        assert len({tuple(m) for m in want}) > 1
    assert play(population(P2.SHAPED, 1, **kw), seeds, moves) == play(population(P2.SHAPED, games, **kw), seeds, moves)


def test_two_rows_play_as_their_own_agents_and_the_refusals(host):
    from agents import PopulationTwoHandAgent
    from agents.greedy import two_hand_agent_class
    from runtime import kernels as K

    seeds, kw = [21, 21, 34, 34], dict(depth=2, candidates=4, deals=3, seed=4)
    sets = [P2.SHAPED, P2.R.DEFAULT_WEIGHTS, P2.R.DEFAULT_WEIGHTS, P2.SHAPED]
    stream = torch.tensor([0, 0, 0, 0], dtype=torch.int64)
    got = play(population(sets, 4, stream=stream, **kw), seeds, 10)
    for e, w in enumerate(sets):  # stream id 0 is what a single-env agent draws from
        alone = play(two_hand_agent_class(w)(w, device="cpu", **kw), [seeds[e]], 10)
        assert [m[e] for m in got] == [m[0] for m in alone], e
    assert [m[0] for m in got] != [m[1] for m in got]
    agent = population(P2.SHAPED, 2, **kw)
    with pytest.raises(NotImplementedError):
        agent.select_action({})
    for bad in (dict(depth=0), dict(candidates=0), dict(candidates=193), dict(deals=0), dict(deals=1025)):
        with pytest.raises(ValueError):
            PopulationTwoHandAgent(K.eval_rows(P2.SHAPED), **{**kw, **bad}, device="cpu")
    with pytest.raises(ValueError):
        PopulationTwoHandAgent(K.weight_rows([P2.R.DEFAULT_WEIGHTS]), device="cpu")
