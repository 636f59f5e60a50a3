"""GPU: the components over several engines (MultiEngine.screen_components_of).  Two engines on ONE device deal the
bands between them, each hooks its own forest, and the forests are joined by one list call: equal to one engine's, field for field."""
import pytest

from tests import screen_cases as scr

pytestmark = pytest.mark.gpu


def test_multi_engine_on_one_device_twice_equals_one_engine():
    from pyani_amd import screen
    from pyani_amd.engine import Engine
    from pyani_amd.multi import MultiEngine
    genomes = scr.family()
    labels = [f"g{i}" for i in range(len(genomes))]
    results = {}
    with Engine(0) as e:
        ids = [e.add_genome(s, o) for s, o in genomes]
        for t in (0.8, 0.999):
            results[t] = e.screen_components_of(ids, screen.ScreenOptions(t, 16, 16), labels=labels, path="index")
    multi = MultiEngine([0, 0])
    try:
        mids = [multi.add_genome(s, o) for s, o in genomes]
        multi.screen_set_band(3)      # three bands dealt to two engines
        for t, one in results.items():
            opt = screen.ScreenOptions(t, 16, 16)
            for path in ("index", "dense"):
                got = multi.screen_components_of(mids, opt, labels=labels, path=path)
                assert got.labels == one.labels
                for f in screen.ScreenComponents._fields[1:]:
                    x, y = getattr(got, f), getattr(one, f)
                    assert x.dtype == y.dtype and x.shape == y.shape and (x == y).all(), (t, path, f)
            assert all(eng.screen_components_last()["n"] == 0 for eng in multi.engines)      # nothing stays resident
    finally:
        multi.close()
    assert len(results[0.8].size) < len(results[0.999].size) and int(results[0.8].entries.sum()) > 0
