"""GPU (through the C ABI): pg_tetra_corr_rows_dev — the row slice of the Pearson matrix that every rank of a multi-GPU TETRA job computes
from the all-gathered Z rows (tetra_stats_kernel, then tetra_pairs_kernel with mirror = 0 and a row offset: pyani_amd/csrc/pg_tetra.hip).
Its only caller is the several-GPU leg of the benchmark, so on one GPU nothing else runs it.  Device buffers come from torch tensors, as
there.  Reference: oracle/tetra_oracle.c (tests/oracle_bind.py), bit for bit; error codes equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 37
CANARY_ROWS = 16
SLICES = [(0, 37), (0, 1), (36, 1), (15, 2), (16, 16), (17, 20), (5, 0)]      # (15, 2) straddles a 16-row tile; (17, 20) ends inside the last one


@pytest.fixture(scope="module")
def eng():
    from pyani_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def z_sets(eng, oracle):
    """{name: (z, present, the oracle's full matrix)}: 'real' from counts of seeded synthetic genomes of 70 ... 130 kb, 'partial' host-made
    (random doubles on one key set of ~100 of the 256 keys).  Computed once, never written to."""
    from pyani_amd import synth
    rng = np.random.default_rng(20260110)
    eng.clear_genomes()
    ids = [eng.add_genome(*synth.genome(20260111, N, g, int(L))) for g, L in enumerate(rng.integers(70_000, 130_001, size=N))]
    z, present, _ = eng.tetra_matrix(ids, want_corr=False)
    eng.clear_genomes()
    assert present.all()
    keys = np.zeros(256, dtype=np.uint8)
    keys[rng.choice(256, size=100, replace=False)] = 1
    pz = rng.normal(0.0, 3.0, size=(N, 256)) * keys
    pp = np.tile(keys, (N, 1))
    out = {}
    for name, (a, p) in {"real": (z, present), "partial": (pz, pp)}.items():
        rc, full = oracle.corr(a, p)
        assert rc == 0 and (np.diag(full) == 1.0).all() and np.abs(full[0, 1:]).max() > 0.0
        a.setflags(write=False); p.setflags(write=False); full.setflags(write=False)
        out[name] = (a, p, full)
    return out


def _rows_dev(eng, z, present, row0, nrows):
    """-> the whole d_out buffer (nrows + CANARY_ROWS rows, NaN before the call) after pg_tetra_corr_rows_dev."""
    import torch
    n = z.shape[0]
    dev = torch.device("cuda", 0)
    d_z = torch.from_numpy(np.array(z, dtype=np.float64)).to(dev)          # (copies: the shared inputs are read-only)
    d_p = torch.from_numpy(np.array(present, dtype=np.uint8)).to(dev)
    d_out = torch.full((nrows + CANARY_ROWS, n), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    eng.tetra_corr_rows_dev(d_z.data_ptr(), d_p.data_ptr(), n, row0, nrows, d_out.data_ptr())
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def _check_slice(eng, z, present, full, row0, nrows):
    n = z.shape[0]
    buf = _rows_dev(eng, z, present, row0, nrows)
    got, canary = buf[:nrows], buf[nrows:]
    assert np.isnan(canary).all(), f"cells written beyond the {nrows} x {n} slice: {np.argwhere(~np.isnan(canary))[:4]}"
    assert not np.isnan(got).any(), f"cells of the slice not written: {np.argwhere(np.isnan(got))[:4]}"
    same = _bits(got) == _bits(full[row0:row0 + nrows])
    assert same.all(), (row0, nrows, np.argwhere(~same)[:4])
    for i in range(row0, row0 + nrows):
        assert got[i - row0, i] == 1.0


@pytest.mark.parametrize("row0,nrows", SLICES)
@pytest.mark.parametrize("name", ["real", "partial"])
def test_row_slices_equal_the_oracle_and_the_full_matrix(eng, z_sets, name, row0, nrows):
    z, present, full = z_sets[name]
    assert (_bits(eng.tetra_corr(z, present)) == _bits(full)).all()
    _check_slice(eng, z, present, full, row0, nrows)


@pytest.mark.parametrize("n", [1, 16, 17])
def test_small_matrices_over_their_full_range(eng, oracle, z_sets, n):
    z, present = z_sets["real"][0][:n], z_sets["real"][1][:n]
    rc, full = oracle.corr(z, present)
    assert rc == 0
    _check_slice(eng, z, present, full, 0, n)


def test_an_empty_slice_on_a_fresh_engine_is_not_an_error(z_sets):
    """A rank without rows (more ranks than genomes).  The flags that PG_E_KEYSET and PG_E_EMPTY are read from are written by the pairs
    kernel, which has nothing to do then; a fresh engine's flags are zero, which once read as 'no tetranucleotide observed'."""
    from pyani_amd.engine import Engine
    z, present, full = z_sets["real"]
    with Engine(0) as fresh:
        _check_slice(fresh, z, present, full, 5, 0)
        _check_slice(fresh, z, present, full, 37, 0)
        _check_slice(fresh, z, present, full, 20, 17)


def test_flags_do_not_depend_on_the_slice(eng, z_sets):
    from pyani_amd import _lib
    z, present, _ = z_sets["partial"]
    odd = present[0].copy()
    odd[np.nonzero(odd)[0][0]] = 0                                  # one key fewer
    for at, (row0, nrows) in ((36, (0, 4)), (0, (0, 4)), (0, (32, 5)), (20, (0, 4)), (20, (36, 1))):      # the offending genome outside and inside the slice
        p = present.copy()
        p[at] = odd
        with pytest.raises(_lib.PyaniGpuError) as ei:
            _rows_dev(eng, z, p, row0, nrows)
        assert ei.value.code == _lib.PG_E_KEYSET, (at, row0, nrows)
    for n in (2, N):
        with pytest.raises(_lib.PyaniGpuError) as ei:
            _rows_dev(eng, np.zeros((n, 256)), np.zeros((n, 256), dtype=np.uint8), 0, 1)
        assert ei.value.code == _lib.PG_E_EMPTY
    for row0, nrows in ((0, N + 1), (N, 1), (30, 8), (2 ** 32 - 1, 2)):
        with pytest.raises(_lib.PyaniGpuError) as ei:
            _rows_dev(eng, z, present, row0, nrows)
        assert ei.value.code == _lib.PG_E_ARG, (row0, nrows)


@pytest.mark.parametrize("between", ["rows_dev", "corr"])
def test_the_cached_batch_survives_a_call_on_unrelated_z(eng, z_sets, between):
    """pg_tetra_matrix keeps its batch's work list while the ids do not change; pg_tetra_corr_rows_dev and pg_tetra_corr overwrite the
    statistics the fused pass leaves on the device.  The same ids again must give the same bits."""
    from pyani_amd import synth
    z, present, full = z_sets["partial"]
    eng.clear_genomes()
    ids = [eng.add_genome(*synth.genome(20260112, 6, g, 80_000 + 1_001 * g)) for g in range(6)]
    first = eng.tetra_matrix(ids)
    if between == "rows_dev":
        _check_slice(eng, z, present, full, 17, 20)
    else:
        assert (_bits(eng.tetra_corr(z, present)) == _bits(full)).all()
    again = eng.tetra_matrix(ids)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    assert (np.diag(first[2]) == 1.0).all() and np.abs(first[2][0, 1:]).min() > 0.0
    eng.clear_genomes()
