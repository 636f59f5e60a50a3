"""MultiEngine.screen_candidates (pyani_amd/multi.py): the devices' parts summed on the host, loaded onto the first engine and selected
there — two engines on device 0 give the candidates one engine gives."""
import numpy as np
import pytest

from tests import screen_cases as scr
from tests import screen_select_cases as ssc


@pytest.mark.gpu
def test_two_engines_on_one_gpu_give_one_engines_candidates():
    from pyani_amd.engine import Engine
    from pyani_amd.multi import MultiEngine
    from pyani_amd.screen import ScreenOptions
    genomes = scr.family()
    labels = [f"g{i}" for i in range(len(genomes))]
    options = [ScreenOptions(t, 16, 16, 2) for t in ssc.THRESHOLDS] + [ScreenOptions(0.9, 12, 16, 1)]
    with Engine(0) as one:
        ids = [one.add_genome(s, o) for s, o in genomes]
        want = [one.screen_candidates(ids, o, labels=labels) for o in options]
    with MultiEngine([0, 0]) as two:
        ids = [two.add_genome(s, o) for s, o in genomes]
        got = [two.screen_candidates(ids, o, labels=labels) for o in options]
    for g, w in zip(got, want):
        assert g.labels == w.labels and g.options == w.options
        for x, y in zip(g[2:], w[2:]):
            assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all()
    counts = [len(w.a) for w in want]
    assert counts[0] == 8 * 7 and 0 < counts[3] < counts[0]
