"""CPU-only: PgDevBuf and PgPinnedBuf (pyani_amd/csrc/pg_devbuf.h), the owning buffers of the library, compiled for the host against
a fake hipMalloc / hipFree / hipHostMalloc / hipHostFree (tests/devbuf/hip/hip_runtime.h) that counts live blocks and fails an
allocation on request."""
import subprocess

from tests.conftest import ROOT


def test_devbuf_never_describes_memory_it_does_not_hold(tmp_path):
    """The ANIm driver's scratch used to keep capacities apart from the pointers they describe; an allocation that failed in the
    middle of a group left a null or too-small array behind a capacity that said otherwise, and the next (smaller) call launched
    kernels on it.  With PgDevBuf: after a failed reserve the buffer is empty (p == nullptr, cap == 0) and a following smaller
    reserve allocates again; a growing reserve frees the old block exactly once; need <= cap allocates nothing; the destructor,
    release() and both moves leave no block live and free none twice.  The pinned buffer follows the same rules.  The context's
    batch scratch (eight arrays, the fourth allocation failing while they grow from 8 to 16 genomes) never reports a size it does not
    hold and is completed by the next call, whatever its size; the arena's replacement (two locals moved into two holders) leaks
    nothing and strands nothing when its second allocation fails."""
    src = ROOT / "tests" / "devbuf"
    exe = tmp_path / "devbuf_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", f"-I{src}", f"-I{ROOT / 'pyani_amd' / 'csrc'}", str(src / "devbuf_check.cpp"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "WRONG" not in out.stdout and out.stdout.count("ok ") == 29, out.stdout
