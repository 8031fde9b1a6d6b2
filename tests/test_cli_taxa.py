"""`panmap <panman> <reads> --meta --filter-and-assign --taxonomic-metadata TSV` (panmap_amd/csrc/cli/panmap_main.cpp): the
three files on rsv_4K against the literal restatement of tests/taxa_checks.py, with a metadata file written from the
labelling -- the reads over the taxon limit are in none of them, the second column names the taxa of the line's head node --
and what the taxonomy options refuse."""
import os
import re
import shutil

import numpy as np
import pytest

import assign_checks as ac
import taxa_checks as tc
from cli_checks import run
from conftest import GOLDEN


def _lines(text):
    out = set()
    for line in text.splitlines():
        ids, taxa, count, idx = line.split("\t")
        idx = [int(x) for x in idx.split(",")]
        assert int(count) == len(idx) and idx == sorted(set(idx))
        out.add((frozenset(ids.split(",")), tuple(taxa.split(",")), frozenset(idx)))
    return out


@pytest.mark.gpu
def test_files_equal_the_restatement(pmx, tmp_path):
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    pm = pmx.Panman(os.path.join(GOLDEN, "rsv_4K.panman"))
    oriented = pmx.Index.build(pm, flank_mask=0, mode=0x100)
    arrays = oriented.arrays()
    parent, n = arrays["parent"], len(arrays["parent"])
    ids = [oriented.node_id(v) for v in range(n)]
    taxon = tc.label(parent, tc.RSV_T)
    names = tc.write_metadata(tmp_path / "meta.tsv", ids, taxon)
    reads = ac.rsv_reads()
    with open(tmp_path / "reads.fastq", "w") as f:
        for i, r in enumerate(reads):
            f.write("@read%d\n%s\n+\n%s\n" % (i, r.decode(), "I" * len(r)))
    r = run(["rsv.panman", "reads.fastq", "--meta", "--filter-and-assign", "--taxonomic-metadata", "meta.tsv", "--maximum-taxon-number", "1",
             "-o", "out"], tmp_path, retry=True)
    assert r.returncode == 0, r.stderr[-2000:]
    want = tc.rsv_leg(arrays)
    n_over, kept = int((want.state == tc.OVER_TAXA).sum()), np.nonzero(want.state == ac.ASSIGNED)[0]
    assert n_over >= 20 and len(kept) >= 20
    assert re.search(r"\(%d assigned, .* %d spanning more than 1 taxa\)" % (len(kept), n_over), r.stderr), r.stderr[-500:]
    # the FASTQ: the kept reads in input order; a read over the limit is in none of the three files
    got_names = [x[1:] for x in open(tmp_path / "out.mgsr.assignedReads.fastq").read().split("\n")[0::4] if x]
    assert got_names == ["read%d" % i for i in kept.tolist()]
    # the lines: (ids of the head and the nodes folded into it, taxon names by ascending taxon index, FASTQ positions)
    heads = ac.heads_np(parent, arrays["offsets"])
    S = tc.subtree_sets(parent, taxon)
    members = {}
    for v in range(n):
        members.setdefault(int(heads[v]), set()).add(ids[v])

    def column(h):
        order = sorted(names.index("tax%d" % t) for t in S[h])
        return tuple(names[i] for i in order) if 0 < len(order) <= 1 else (".",)

    by_node, by_lca = {}, {}
    for pos, raw in enumerate(kept.tolist()):
        for h in {int(heads[v]) for v in want.nodes[raw]}:
            by_node.setdefault(h, set()).add(pos)
        by_lca.setdefault(int(heads[want.lca[raw]]), set()).add(pos)
    for path, groups in (("out.mgsr.assignedReads.out", by_node), ("out.mgsr.assignedReadsLCANode.out", by_lca)):
        want_lines = {(frozenset(members[h]), column(h), frozenset(g)) for h, g in groups.items()}
        assert _lines(open(tmp_path / path).read()) == want_lines, path
        assert any(t != (".",) for _, t, _ in want_lines) and any(t == (".",) for _, t, _ in want_lines)


def test_refusals(tmp_path):
    shutil.copy(os.path.join(GOLDEN, "rsv_4K.panman"), tmp_path / "rsv.panman")
    (tmp_path / "r.fastq").write_text("@a\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    (tmp_path / "meta.tsv").write_text("id\tGenus\tFamily\nnode_1\tG\tF\n")
    base = ["rsv.panman", "r.fastq", "--meta", "--filter-and-assign"]
    with_file = base + ["--taxonomic-metadata", "meta.tsv"]
    for args, words in ((with_file + ["--discard", "0.5", "--ambiguous-score-threshold", "2"], "cannot be combined"),
                        (with_file + ["--discard", "0.5", "--ambiguous-score-threshold-ratio", "0.1"], "cannot be combined"),
                        (with_file + ["--maximum-taxon-number", "17"], "between 1 and 16"),
                        (with_file + ["--maximum-taxon-number", "0"], "between 1 and 16"),
                        (with_file + ["--taxonomic-rank", "Order"], "'Order' not found"),
                        (with_file + ["--taxonomic-rank", "id"], "first column"),
                        (base + ["--taxonomic-rank", "Genus"], "option --taxonomic-rank is not accepted without --taxonomic-metadata"),
                        (base + ["--ambiguous-score-threshold-ratio", "0.1"], "is not accepted without --taxonomic-metadata"),
                        (base + ["--taxonomic-metadata", "absent.tsv"], "option --taxonomic-metadata is not accepted: cannot read absent.tsv"),
                        (["rsv.panman", "r.fastq", "--meta", "--taxonomic-metadata", "meta.tsv"], "is not accepted without --filter-and-assign"),
                        (with_file + ["--jplace"], "not accepted"), (with_file + ["--breadth-ratio", "0.5"], "not accepted"),
                        (with_file + ["--mask-read-ends", "3"], "not accepted")):
        r = run(args, tmp_path, retry=True)
        assert r.returncode == 1 and words in r.stderr, (args, r.stderr[-300:])
