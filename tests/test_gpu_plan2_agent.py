"""``PopulationTwoHandAgent`` on the GPU: equal rows play ``TwoHandShapeAgent``'s 8 envs x 12 moves and its own moves
on the host backend; with two different rows each env plays as its own single-set agent."""
import pytest
import torch

import _plan2_ref as P2
from _plan2_ref import play, population

pytestmark = pytest.mark.gpu


def test_equal_rows_play_the_shape_agent_and_the_host_backend(cuda, lib):
    from agents.greedy import TwoHandShapeAgent
    from runtime.build import build_host_lib

    build_host_lib(verbose=False)
    seeds, kw = list(range(50, 58)), dict(depth=3, candidates=4, deals=4, seed=6)
    want = play(TwoHandShapeAgent(P2.SHAPED, device=cuda, **kw), seeds, 12, device=cuda)
    assert play(population(P2.SHAPED, 8, device=cuda, **kw), seeds, 12, device=cuda) == want
    assert play(population(P2.SHAPED, 8, device="cpu", **kw), seeds, 12, device="cpu") == want
    assert len({tuple(m) for m in want}) > 6


def test_two_rows_play_as_their_own_agents(cuda, lib):
    from agents.greedy import two_hand_agent_class

    seeds, kw = [21, 21, 34, 34], dict(depth=2, candidates=4, deals=3, seed=4)
    sets = [P2.SHAPED, P2.R.DEFAULT_WEIGHTS, P2.R.DEFAULT_WEIGHTS, P2.SHAPED]
    stream = torch.zeros(4, dtype=torch.int64, device=cuda)
    got = play(population(sets, 4, device=cuda, stream=stream, **kw), seeds, 10, device=cuda)
    for e, w in enumerate(sets):
        alone = play(two_hand_agent_class(w)(w, device=cuda, **kw), [seeds[e]], 10, device=cuda)
        assert [m[e] for m in got] == [m[0] for m in alone], e
    assert [m[0] for m in got] != [m[1] for m in got]
