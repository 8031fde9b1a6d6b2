"""bench.py's host-side helpers without a GPU: the threaded workload generator and the --dump-outputs format."""
import importlib.util
import os
import types

import numpy as np

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_threaded_workload_equals_one_call(pmx):
    """the reads of the benchmark's workload are those of one simulate_paired_reads_8d call, whatever the stretches"""
    from panmap_amd import synth
    bench = _bench()
    genome = b"ACGTTGCAAGGCTTAACCGGTA" * 200
    for n_pairs, first in ((1100003, 0), (500001, 777)):
        a, ao = synth.simulate_paired_reads_8d(genome, n_pairs, first_pair=first, read_len=100, seed=42)
        b, bo = bench.simulate_pairs_8d(synth, genome, n_pairs, first, 100, 42)
        assert np.array_equal(a, b) and np.array_equal(ao, bo)


def _outputs(pmx, n, n_cigar):
    rng = np.random.default_rng(5)
    recs = np.zeros(n, pmx.REC_DTYPE)
    for f in ("rs", "re", "qs", "qe", "score"):
        recs[f] = rng.integers(0, 30000, n)
    recs["mapped"] = 1
    recs["n_cigar"] = n_cigar
    recs["cigar_off"] = np.cumsum(recs["n_cigar"].astype(np.int64)) - recs["n_cigar"]
    arena = rng.integers(0, 1 << 31, int(recs["n_cigar"].astype(np.int64).sum()), dtype=np.uint32)
    res = types.SimpleNamespace(best_score=[1.5, 2.0, 3.0, 4.0, -5.25], best_index=[3, 4, 5, 6, 7],
                                tied_indices=[np.array([3]), np.array([4, 9]), np.array([5]), np.array([6]), np.array([7, 8])])
    return recs, arena, res, rng.random((1000, 5))


def test_dump_outputs_format(pmx, tmp_path):
    bench = _bench()
    recs, arena, res, scores = _outputs(pmx, 300000, 3)
    bench.dump_outputs(str(tmp_path / "a"), recs, arena, res, scores)
    bench.dump_outputs(str(tmp_path / "b"), recs, arena, res, scores)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(got) == {"records", "record_index", "cigar_ops", "placement", "ties", "node_scores"}
    assert all(a.dtype == np.float64 for a in got.values())
    for k, a in got.items():                                             # a fixed sample: the same from call to call
        assert np.array_equal(a, np.load(tmp_path / "b" / (k + ".npy"))), k
    idx = got["record_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_RECORDS and np.all(np.diff(idx) > 0)
    assert np.array_equal(got["records"][:, 0], recs["rs"][idx]) and np.array_equal(got["records"][:, 10], recs["score"][idx])
    ops = np.concatenate([arena[recs["cigar_off"][i]:recs["cigar_off"][i] + 3] for i in idx[:5]])
    assert np.array_equal(got["cigar_ops"][:15], ops)
    assert got["placement"].tolist() == [[1.5, 3], [2.0, 4], [3.0, 5], [4.0, 6], [-5.25, 7]]
    assert got["ties"].tolist() == [[0, 3], [1, 4], [1, 9], [2, 5], [3, 6], [4, 7], [4, 8]]


def test_dump_outputs_stays_within_64mb(pmx, tmp_path):
    """long reads: the CIGARs of the sample would pass 64 MB, so the sample is cut short"""
    bench = _bench()
    recs, arena, res, scores = _outputs(pmx, 50000, 400)
    bench.dump_outputs(str(tmp_path), recs, arena, res, scores)
    total = sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path))
    assert 60 << 20 < total <= 64 << 20
    got = np.load(tmp_path / "records.npy")
    assert len(np.load(tmp_path / "cigar_ops.npy")) == 400 * len(got) < 400 * 50000
