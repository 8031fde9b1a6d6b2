"""The host side of --amplicon-depth: the table parser through the C ABI (pmx_amplicons_*, by load_amplicons) against the file
rules of extractReadSequences (src/mgsr.cpp:1216-1342) as tests/amplicon_checks.py restates them.  No device."""
import numpy as np
import pytest

import amplicon_checks as amp

ERR_IO, ERR_FORMAT = -2, -3


def _error(pmx, path):
    with pytest.raises(pmx._lib.PmxError) as err:
        pmx.load_amplicons(str(path))
    return err.value


def test_parser_follows_the_rules(pmx, tmp_path):
    text = "r1\tP2\n\nr2\tP1\nr3\tP2\r\nr1\tP3\n\n\nr4\tP_only_for_r2\nr4\tP1\nr5 with a blank\tP3"      # (no newline at the end)
    (tmp_path / "depth.tsv").write_text(text, newline="")
    want_names, want_of = amp.parse_table(text)
    a = pmx.load_amplicons(str(tmp_path / "depth.tsv"))
    assert a.names == want_names == ["P2", "P1", "P3", "P_only_for_r2"]                 # numbered by first appearance
    assert a.lookup("r1") == 2 and want_of["r1"] == 2                                   # the last line of a read id counts
    assert a.lookup("r4") == 1 and 3 not in want_of.values()                            # ... and leaves an empty group behind
    assert a.lookup("r3") == 0 and a.lookup("r5 with a blank") == 2
    assert a.lookup("never_listed") == -1 and a.lookup("") == -1 and a.lookup("P1") == -1
    names = ["r1", "r2", "nobody", "r3", "r4"]
    got = a.groups_of(names)
    assert got.dtype == np.int32 and np.array_equal(got, amp.groups_of(names, 4, want_of)) and got.tolist() == [2, 1, 4, 0, 1]


def test_the_family_table(pmx, tmp_path):
    D = amp.family()
    (tmp_path / "family.tsv").write_text(D.table)
    a = pmx.load_amplicons(str(tmp_path / "family.tsv"))
    assert a.names == D.group_names
    assert np.array_equal(a.groups_of(D.names), D.groups) and a.lookup("not_in_the_sample") == 3


def test_an_empty_file_has_no_groups(pmx, tmp_path):
    (tmp_path / "empty.tsv").write_text("\n\n")
    a = pmx.load_amplicons(str(tmp_path / "empty.tsv"))
    assert a.names == [] and a.groups_of(["x", "y"]).tolist() == [0, 0]


def test_error_codes(pmx, tmp_path):
    assert _error(pmx, tmp_path / "absent.tsv").code == ERR_IO
    assert _error(pmx, tmp_path).code == ERR_IO                                          # a directory
    for i, bad in enumerate(("r1\tP1\n\nr2 P1\n", "r1\tP1\n\nr2\tP1\tmore\n", "r1\tP1\n\n\tP1\n", "r1\tP1\n\nr2\t\n")):
        path = tmp_path / ("bad%d.tsv" % i)
        path.write_text(bad)
        err = _error(pmx, path)
        assert err.code == ERR_FORMAT and "line 3" in str(err), bad
        with pytest.raises(ValueError, match="3"):
            amp.parse_table(bad)
