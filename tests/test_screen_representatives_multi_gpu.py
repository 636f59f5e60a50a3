"""GPU: the greedy representatives over several engines (MultiEngine.screen_dereplicate).  Two engines on ONE device deal
the candidates between them as today and ONE list call runs on the first engine: equal to one engine's, field for field."""
import numpy as np
import pytest

from tests import screen_cases as scr

pytestmark = pytest.mark.gpu


def test_multi_engine_on_one_device_twice_equals_one_engine():
    from pyani_amd import screen
    from pyani_amd.engine import Engine
    from pyani_amd.multi import MultiEngine
    genomes = scr.family()
    labels = [f"g{i}" for i in range(len(genomes))]
    given = np.random.default_rng(3).random(len(genomes)) * 100.0
    results = {}
    with Engine(0) as e:
        ids = [e.add_genome(s, o) for s, o in genomes]
        for t in (0.8, 0.999):
            for scores in (None, given):
                results[t, scores is None] = e.screen_dereplicate(ids, screen.ScreenOptions(t, 16, 16), scores=scores, labels=labels, path="index")
    multi = MultiEngine([0, 0])
    try:
        mids = [multi.add_genome(s, o) for s, o in genomes]
        multi.screen_set_band(3)      # three bands dealt to two engines
        for (t, sizes_win), one in results.items():
            opt = screen.ScreenOptions(t, 16, 16)
            for path in ("index", "dense"):
                got = multi.screen_dereplicate(mids, opt, scores=None if sizes_win else given, labels=labels, path=path)
                assert got.labels == one.labels
                for f in screen.ScreenClusters._fields[1:]:
                    x, y = getattr(got, f), getattr(one, f)
                    assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), (t, path, f)
            assert all(eng.screen_representatives_last()["n"] == 0 for eng in multi.engines)      # nothing stays resident
        a, b = np.array([0, 1], np.int32), np.array([1, 2], np.int32)
        rep, via = multi.screen_representatives(a, b, np.array([3, 9], np.uint32), n=3, score=np.array([10, 5, 1], np.uint64))
        assert rep.tolist() == [0, 2, 2] and via.tolist() == [0, 9, 0]
        multi.screen_representatives_release()
    finally:
        multi.close()
    assert len(results[0.8, True].size) < len(results[0.999, True].size)
