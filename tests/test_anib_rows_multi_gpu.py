"""MultiEngine.anib_rows_batch: two engines on one device give exactly what one engine gives."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_two_engines_on_one_gpu_equal_one_engine():
    from pyani_amd import synth
    from pyani_amd.engine import Engine
    from pyani_amd.multi import MultiEngine
    n, L, seed = 8, 30_000, 31
    data = [synth.genome(seed, n, g, L) for g in range(n)]
    pairs = [(a, b) for a in range(n) for b in range(n) if a != b]
    pairs = [pairs[k] for k in np.random.RandomState(3).permutation(len(pairs))[:40]]
    with Engine(0) as one:
        ids = [one.add_genome(*d) for d in data]
        want = one.anib_rows_batch([ids[a] for a, _ in pairs], [ids[b] for _, b in pairs])
    with MultiEngine([0, 0], chunk_pairs=8) as two:
        ids2 = [two.add_genome(*d) for d in data]
        assert ids2 == ids
        got = two.anib_rows_batch([ids[a] for a, _ in pairs], [ids[b] for _, b in pairs])
    assert got[0].dtype == want[0].dtype and got[0].tobytes() == want[0].tobytes()
    assert np.asarray(got[1]).tolist() == np.asarray(want[1]).tolist() and int(want[1][-1]) > 500
    assert got[2].dtype == want[2].dtype and got[2].tobytes() == want[2].tobytes()
