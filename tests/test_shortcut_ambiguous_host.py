"""The DP shortcuts' closed forms over ambiguous bases (align/aln_ksw.hpp: ksw_shortcut_ext_amb, ksw_shortcut_fill_decide)
against the host build of ksw_extd2, on N-heavy problems."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "shortcut_amb.cpp")
INC = os.path.join(HERE, "..", "panmap_amd", "csrc")


_LIB = []


def _lib(tmp_path_factory):
    if _LIB:
        return _LIB[0]
    out = str(tmp_path_factory.mktemp("shortcut_amb") / "libshortcut_amb.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
                    "-Wno-unknown-pragmas", "-I" + INC, SRC, "-o", out], check=True)
    L = C.CDLL(out)
    L.hs_amb_shortcut_fuzz.restype = C.c_int
    L.hs_amb_shortcut_fuzz.argtypes = [C.c_uint64, C.c_int64, C.POINTER(C.c_int64), C.c_int]
    _LIB.append(L)
    return L


def test_ambiguous_shortcuts_against_the_dp_fuzz(tmp_path_factory):
    """runs of 1-40 N on the query, the target or both, 0-3 substitutions, extensions and fills of both gap alignments:
    every answer the shortcuts give equals the DP's, and a good share of the N-bearing problems is answered"""
    L = _lib(tmp_path_factory)
    counts = (C.c_int64 * 4)()
    L.hs_amb_shortcut_fuzz(2024, 2000000, counts, 1)
    declined, agreed, bad, agreed_amb = counts[0], counts[1], counts[2], counts[3]
    assert bad == 0, (declined, agreed, bad)
    assert agreed_amb > 200000, (declined, agreed, agreed_amb)


def test_fill_over_n_runs_keeps_the_zdrop_test(tmp_path_factory):
    """a gap fill over an N run answered by the shortcut can drop by more than zdrop (sc_ambi per N): align1's fill step
    (shortcut, fill_zdrop_skip, test_zdrop, second pass) must end where the same step with the DP ends, for the short-
    and the long-read preset, and a skipped test_zdrop must be one that returns 0"""
    L = _lib(tmp_path_factory)
    L.hs_amb_fill_zdrop.restype = C.c_int
    L.hs_amb_fill_zdrop.argtypes = [C.c_uint64, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int]
    for preset, max_run in ((0, 150), (1, 500)):
        counts = (C.c_int64 * 4)()
        L.hs_amb_fill_zdrop(99, 3000, preset, max_run, counts, 1)
        answered, differing, bad_skips, fired = counts[0], counts[1], counts[2], counts[3]
        assert differing == 0 and bad_skips == 0, (preset, answered, differing, bad_skips, fired)
        assert answered > 1000 and fired > 200, (preset, answered, fired)
