"""The host side of the taxonomy filter: the metadata parser (pmx_taxonomy_load through load_taxonomy) against the rules of
loadTaxonomicMetadata (src/mgsr.cpp:198-256) on the crafted file of tests/taxa_checks.py, with every error code; and the
subtree taxon sets a Meta keeps (pmx_meta_node_taxa) against taxa_checks.subtree_sets.  The parser needs no device; a Meta
does, so the last test is a `gpu` one."""
import numpy as np
import pytest

import assign_checks as ac
import taxa_checks as tc

ERR_ARG, ERR_IO, ERR_FORMAT = -1, -2, -3


def _code(pmx, path, rank="Family"):
    with pytest.raises(pmx._lib.PmxError) as err:
        pmx.load_taxonomy(str(path), rank, ["a"])
    return err.value.code


def test_parser_follows_the_reference_rules(pmx, tmp_path):
    parent = ac.crafted_trees()[tc.TREES["random300"]].parent
    taxon = tc.label(parent, 16)
    ids = ["node_%d" % v for v in range(len(parent))]
    want_names = tc.write_metadata(tmp_path / "meta.tsv", ids, taxon)
    names, got = pmx.load_taxonomy(str(tmp_path / "meta.tsv"), "Family", ids + ["never_listed"])
    assert names == want_names and names[:2] == ["elsewhere", "overwritten"]     # first appearance, unknown identifiers included
    assert got.dtype == np.int32 and got[-1] == -1
    for v in range(len(parent)):                                                   # `.` rows and unlisted nodes: none; the later row counts
        assert got[v] == (names.index("tax%d" % taxon[v]) if taxon[v] >= 0 else -1), v
    assert (taxon < 0).any() and (taxon >= 0).sum() > 100
    # another column of the same file: the decoy is a taxonomy of its own
    genus, g = pmx.load_taxonomy(str(tmp_path / "meta.tsv"), "Genus", ids)
    assert set(genus) == {"x"} | {"tax%d" % i for i in range(7)} and (g >= 0).sum() == (taxon >= 0).sum() + 1   # (+ the `.` row's node)
    order, o = pmx.load_taxonomy(str(tmp_path / "meta.tsv"), "Order", ids)
    assert "y" in order and "decoy5" in order


def test_parser_error_codes(pmx, tmp_path):
    (tmp_path / "ok.tsv").write_text("id\tFamily\na\tF1\n")
    assert pmx.load_taxonomy(str(tmp_path / "ok.tsv"), "Family", ["a", "b"])[1].tolist() == [0, -1]
    assert _code(pmx, tmp_path / "absent.tsv") == ERR_IO
    assert _code(pmx, tmp_path) == ERR_IO                                          # a directory
    assert _code(pmx, tmp_path / "ok.tsv", "Genus") == ERR_ARG                     # no such rank
    assert _code(pmx, tmp_path / "ok.tsv", "id") == ERR_ARG                        # the identifier column
    (tmp_path / "short.tsv").write_text("id\tGenus\tFamily\na\tG1\tF1\nb\tG2\n")
    assert _code(pmx, tmp_path / "short.tsv") == ERR_FORMAT
    assert pmx.load_taxonomy(str(tmp_path / "short.tsv"), "Genus", ["b"])[1].tolist() == [1]
    (tmp_path / "empty.tsv").write_text("")
    assert _code(pmx, tmp_path / "empty.tsv") == ERR_FORMAT


@pytest.mark.gpu
@pytest.mark.parametrize("max_taxa", [1, 2, 8])
def test_node_taxa_are_the_subtree_sets(pmx, max_taxa):
    tree = ac.crafted_trees()[tc.TREES["random300"]]
    plain, oriented = tree.indexes(pmx)
    meta = pmx.Meta(pmx.Context(0), plain, oriented)
    taxon = tc.label(tree.parent, 16)
    meta.set_taxonomy(taxon, max_taxa)
    S = tc.subtree_sets(tree.parent, taxon)
    sizes = set()
    for v in range(len(tree.parent)):
        got = meta.node_taxa(v)
        assert (got is None) == (len(S[v]) > max_taxa), v
        if got is not None:
            assert got.tolist() == sorted(S[v]), v
            sizes.add(len(got))
    assert sizes >= set(range(min(max_taxa, 3) + 1)) and meta.node_taxa(0) is None
    # a head's set covers the nodes folded into it: S is taken before identical nodes are folded
    heads = oriented.node_heads()
    folded = [v for v in range(len(heads)) if heads[v] != v and S[v] and len(S[heads[v]]) <= max_taxa]
    assert folded or max_taxa == 1
    for v in folded:
        assert S[v] <= set(meta.node_taxa(int(heads[v])).tolist())
    with pytest.raises(ValueError):
        meta.node_taxa(len(heads))
    meta.set_taxonomy(max_taxa=0)
    with pytest.raises(ValueError):
        meta.node_taxa(0)
    meta.close()
