"""The chain fill's dominated tail (align/aln_compact.hpp) on read pairs whose mates overlap on the reference, in the host
build of the kernel source (tests/hostsim), CPU only: 2,048 pairs per case of tests/chain_overlap_cases.py.

Every pair a form of the compact tier finishes must carry the record of the reference's own aligner (oracle/_ref), and the
set of finished pairs must be the one the commit before the dominated tail finished: a closed form that changed which pairs
the tier finishes would shrink (or shift) the comparison unnoticed.  PARENT_DONE holds, per case and form, the count and the
SHA-1 of the parent's `done` array (int8, one per pair), taken from the parent's host build; PARENT_TRIPS_CLEAN is the
parent's mean number of predecessor-loop trips per pair of the error-free case (hs_compact_trace), which the dominated
tail has to undercut -- it must fire, not merely be harmless.

The indel case finishes 34 % of its pairs (30 % in the first form), under the 80 % a case should reach: 1,366 of the 2,048
pairs carry a read with an indel and the compact tier hands gapped pairs on to the general tiers whatever the insert size
(inserts of 200-290, 290-400 and 400-500 finish 682 pairs, none of them gapped), so no other insert range helps and the
case keeps the inserts of the other two.  The first form finishes 75 % of the substituted case (the second form 96 %)."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import align_checks as ac
from chain_overlap_cases import CASES, overlap_pairs

N_PAIRS = 2048
FORMS = {
    "first": {},
    "second": {"PMX_HS_COMPACT_MULTI": "1"},
    "pos32": {"PMX_HS_COMPACT_POS32": "1", "PMX_HS_COMPACT_MULTI": "1"},
}
PARENT_DONE = {
    ("clean", "first"): (1781, "b4c0692332156ed4541e470651414207e7293d64"),
    ("clean", "second"): (2048, "26ad4b31297bba77aef87b93bf185e908d26b101"),
    ("clean", "pos32"): (2048, "26ad4b31297bba77aef87b93bf185e908d26b101"),
    ("subs", "first"): (1543, "5bf0229e999bdfff68ec32f07a09ddc5fc9ab48d"),
    ("subs", "second"): (1975, "5e5176b821560b28b68d5fa8c3939c3f13f65b32"),
    ("subs", "pos32"): (1975, "5e5176b821560b28b68d5fa8c3939c3f13f65b32"),
    ("indel", "first"): (609, "b841c8ebe8ba23b3dd172010796c4d0a7c9c4d5c"),
    ("indel", "second"): (695, "ed8bb1782deb4b81c6cb9522084423c7b79f25a5"),
    ("indel", "pos32"): (695, "ed8bb1782deb4b81c6cb9522084423c7b79f25a5"),
}
PARENT_TRIPS_CLEAN = {"first": 749.213, "second": 749.686, "pos32": 749.686}

_cache = {}


def _case(sars, oracle, case):
    if case not in _cache:
        g = sars.genome("node_7618")
        reads = overlap_pairs(g, case, N_PAIRS)
        _cache[case] = (g, reads, oracle.ref_align_reads_direct(g, reads, True, 8))
    return _cache[case]


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("case", CASES)
def test_overlapping_mates_equal_reference_and_parent_done(sars, oracle, case, form, monkeypatch):
    for k in ("PMX_HS_COMPACT_MULTI", "PMX_HS_COMPACT_SPLIT", "PMX_HS_COMPACT_POS32"):
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    g, reads, want = _case(sars, oracle, case)
    L = ac.hostsim(False)
    L.hs_compact_trace.argtypes = [C.c_void_p]
    trace = np.zeros((N_PAIRS, 129), np.uint8)
    L.hs_compact_trace(trace.ctypes.data)
    try:
        got, done = ac.hostsim_align_compact(g, reads)
    finally:
        L.hs_compact_trace(None)
    digest = hashlib.sha1(done.astype(np.int8).tobytes()).hexdigest()
    trips = float(trace[:, 1:65].astype(np.int64).sum(1).mean())
    print("%s %s: done %d %s, mean trips per pair %.3f" % (case, form, int(done.sum()), digest, trips))
    idx = [i for i in range(N_PAIRS) if done[i]]
    bad = ac.compare_results([got[i] for i in idx], [want[i] for i in idx])
    assert not bad, (case, form, bad[:5])
    assert (int(done.sum()), digest) == PARENT_DONE[case, form]
    if case == "clean":
        assert trips < PARENT_TRIPS_CLEAN[form]
