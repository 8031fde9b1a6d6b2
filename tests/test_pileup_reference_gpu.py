"""The device pileup against the reference's own programs: crafted read sets (tests/golden/pileup_crafted_inputs.json.gz) go
through Pileup.run_records -- the path rank 0 of a `--gpus N` run takes -- and the tables are compared cell for cell with
the numpy restatement, and, through what an mpileup record states, with the recorded output of `bcftools mpileup -B` at
every position; the records pmx.Genotyper writes from them with the recorded `bcftools call` lines.  The demo reads do the
same through the aligner's resident results.  Reads only tests/golden."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import geno_checks as gc
import pileup_golden as pg
from test_pileup_reference import LEGS, check_preconditions, leg_set


def _run_records(pmx, ctx, ds, params, revcomp_mate2=False):
    reads, quals = ds["reads"], ds["quals"]
    if revcomp_mate2:   # mate 2 as the sequencer gives it: the pipeline reverse-complements it before it aligns
        reads = [r if i % 2 == 0 else pmx.reverse_complement(r) for i, r in enumerate(reads)]
        quals = [q if i % 2 == 0 else q[::-1] for i, q in enumerate(quals)]
    concat, off = pmx.concat_reads(reads)
    pu = pmx.Pileup(ctx)
    pu.run_records(ds["recs"], ds["cig"], concat, off, len(ds["ref"]), ds["paired"], revcomp_mate2, quals=b"".join(quals), names=ds["names"],
                   params=pmx.PileupParams(**params))
    hist, aux = pu.tables()
    flags, rank = pu.read_info()
    pu.close()
    return hist, aux, flags, rank


def _check_leg(pmx, ctx, leg_name, leg, ds, tmp_path):
    want_rank = pg.bam_order(pmx, ds, str(tmp_path / (leg_name + ".bam")))
    hist, aux, flags, rank = _run_records(pmx, ctx, ds, leg["params"])
    assert np.array_equal(rank, want_rank), "read_info() rank is not the BAM's order"
    concat, off = pmx.concat_reads(ds["reads"])
    w_hist, w_aux, info = gc.pileup_tables(ds["recs"], ds["cig"], concat, off, len(ds["ref"]), ds["paired"], False, want_rank,
                                           quals=b"".join(ds["quals"]), names=ds["names"], **leg["params"])
    info["features"] = gc.features(ds["recs"], ds["cig"], np.frombuffer(concat, np.uint8), off, ds["paired"])
    print(leg_name, {k: v for k, v in info.items() if k not in ("admitted", "late_reads")})
    check_preconditions(leg_name, leg, w_hist, info)
    assert np.array_equal((flags & 1).astype(bool), info["admitted"])
    assert int(((flags & 2) != 0).sum()) == 2 * info["reconciled_pairs"]
    assert np.array_equal(aux, w_aux), "aux differs at positions %s" % np.nonzero((aux != w_aux).any(axis=1))[0][:10]
    bad = np.nonzero((hist != w_hist).reshape(len(ds["ref"]), -1).any(axis=1))[0]
    assert bad.size == 0, "hist differs at %d positions, first %s" % (bad.size, bad[:10])
    assert hist.sum(axis=(1, 2, 3)).max() <= 255
    diff = pg.compare_with_mpileup(leg, hist, aux, ds["ref"], pmx.site_call)
    assert not diff, "%d positions differ from mpileup, first %s" % (len(diff), diff[:5])
    for name, phred in pg.spectra().items():
        assert pmx.Genotyper(hist, aux, ds["ref"], pg.CHROM, phred).records() == pg.expected_records(pmx, leg, phred), name
    if ds["paired"]:
        h2, a2, _, r2 = _run_records(pmx, ctx, ds, leg["params"], revcomp_mate2=True)
        assert np.array_equal(r2, rank) and np.array_equal(a2, aux) and np.array_equal(h2, hist), "mate 2 handed over un-reversed gives other tables"


@pytest.mark.gpu
@pytest.mark.parametrize("leg_name", LEGS)
def test_crafted_records_through_the_device_pileup(pmx, ctx, leg_name, tmp_path):
    """edges_reversed is the edges set with its pairs in the opposite order (another BAM order of equal starts)"""
    leg, ds = leg_set(leg_name)
    _check_leg(pmx, ctx, leg_name, leg, ds, tmp_path)


@pytest.mark.gpu
def test_demo_device_tables_equal_mpileup_at_every_record(pmx, ctx):
    """one alignment of the demo reads: the resident-results path and run_records on the fetched records give the same
    tables, and those state what the reference's mpileup recorded at all 29,514 records"""
    import test_genotype_gpu as tg
    genome = tg._genome()
    ds = tg._isolate_set(pmx)
    got = tg._pileup(pmx, ctx, genome, ds, 250)
    leg = pg.demo_leg()
    assert len(leg["mpileup"]["pos"]) == 29514 and leg["n_indel"] == 8
    assert got["hist"].sum(axis=(1, 2, 3)).max() <= 255
    diff = pg.compare_with_mpileup(leg, got["hist"], got["aux"], genome, pmx.site_call)
    assert not diff, "%d positions differ from mpileup, first %s" % (len(diff), diff[:5])
    concat, off = pmx.concat_reads(got["reads"])
    pu = pmx.Pileup(ctx)
    pu.run_records(got["recs"], got["cig"], concat, off, len(genome), True, True, quals=b"".join(got["quals"]), names=got["names"])
    hist, aux = pu.tables()
    flags, rank = pu.read_info()
    assert np.array_equal(hist, got["hist"]) and np.array_equal(aux, got["aux"])
    assert np.array_equal(flags, got["flags"]) and np.array_equal(rank, got["rank"])
    counts, branches, length = pmx.spectrum_counts(pmx.Panman(os.path.join(GOLDEN, "sars_20000_twilight_dipper.panman")))
    for phred in [pmx.spectrum_phred(counts, branches, length)] + list(pg.spectra().values()):
        assert pmx.Genotyper(hist, aux, genome, "node_7618", phred).records() == pg.expected_records(pmx, leg, phred)
