"""--meta over several GPUs, the parts that need no GPU: the C ABI entry points exist and check their arguments, and a rank
of `panmap --meta --gpus N` that fails ends the run (the reaping the place path has)."""
import ctypes as C
import os
import shutil
import time

from cli_checks import run
from conftest import GOLDEN



def test_attach_dist_and_row_range_are_in_the_abi(pmx):
    from panmap_amd._lib import lib
    assert lib.pmx_meta_attach_dist(None, None) != 0
    first, count = C.c_int64(-1), C.c_int64(-1)
    assert lib.pmx_meta_row_range(None, C.byref(first), C.byref(count)) != 0
    assert hasattr(pmx.Meta, "attach_dist") and hasattr(pmx.Meta, "row_range")


def test_a_failing_meta_rank_ends_the_run(pmx, tmp_path):
    """every rank asks for a device ordinal the box does not have: the run ends with a non-zero code, soon, and leaves no
    rendezvous behind"""
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    (tmp_path / "r.fastq").write_text("@a\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    env = dict(os.environ, PMX_DEVICE="63")
    t0 = time.time()
    r = run(["rsv.panman", "r.fastq", "--meta", "--gpus", "2"], tmp_path, env=env, timeout=120)
    assert r.returncode != 0 and time.time() - t0 < 60, (r.returncode, r.stderr[-500:])
    assert "opening the GPU" in r.stderr, r.stderr[-500:]
    assert not [d for d in os.listdir("/tmp") if d.startswith("panmap_ranks_") and os.path.exists(os.path.join("/tmp", d, "uid"))]
    r = run(["rsv.panman", "r.fastq", "--meta", "--gpus", "2", "-l", "1"], tmp_path, timeout=120)
    assert r.returncode == 1 and "--meta needs l >= 2" in r.stderr
