"""Node scoring on crafted trees (tests/place_tree_checks.py), in every form of the scoring pass: the heavy-path chains kernel,
the flag-per-node kernel, the level kernels replayed from a graph and as plain launches, and the level-kernel redo after a
starved persistent launch.  Every case is compared with the oracle bit for bit, and Placer.score_info() must name the path the
call took: a withheld or late flag ends in the redo, whose result is bit-exact again -- only `redone` shows it."""
import numpy as np
import pytest

import place_tree_checks as tc

pytestmark = pytest.mark.gpu

_indexes = {}


def _index(pmx, name):
    if name not in _indexes:
        _indexes[name] = tc.tree(name).index(pmx)
    return _indexes[name]


def _set_form(monkeypatch, form):
    for sw in ("PMX_PLACE_TREE_KERNEL", "PMX_PLACE_LEVEL_KERNELS", "PMX_PLACE_NO_GRAPH", "PMX_PLACE_TEST_STARVED"):
        monkeypatch.delenv(sw, raising=False)
    for sw in tc.FORMS[form][0]:
        monkeypatch.setenv(sw, "1")


def _score_and_check(pmx, placer, name, form, hist="A", params=None):
    """reset, merge, score; the result against the oracle and the path against the form asked for"""
    params = params or pmx.TraversalParams()
    keys, counts = tc.histogram(hist)
    placer.reset()
    if len(keys):
        placer.merge(keys, counts)
    res = placer.score(params, 0)
    info = placer.score_info()
    print(name, form, hist, info)
    want = tc.want(name, hist, params.seedMaskFraction, params.minReadSupport, params.forceLeaf)
    tc.assert_place_matches(placer, res, want)
    d = tc.decomposition(name)
    assert info["form"] == tc.FORMS[form][1]
    assert (info["n_chains"], info["max_chain_len"], info["n_levels"]) == (d["n_chains"], d["max_chain_len"], d["n_levels"])
    if form == "starved":
        assert info["redone"] == 1, "PMX_PLACE_TEST_STARVED did not lead to the level-kernel redo"
    else:
        assert info["redone"] == 0, ("the persistent launch reported a starved grid and the scoring was redone with the level kernels: "
                                     "either the grid really was not resident (another process on the GPU), or a flag was withheld or "
                                     "published late and a wave polled to its limit")
    if info["form"] in ("chains", "tree"):
        assert info["grid_waves"] >= 4 and info["grid_waves"] % 4 == 0
    if info["form"] == "chains" and name in ("star", "random"):
        # these shapes exist to make every wave take a second, third and fourth chain: on a card with more CUs than the 256
        # they assume this fails, and the shapes must be enlarged
        assert info["n_chains"] > 3 * info["grid_waves"], info
    return res, want, info


@pytest.mark.parametrize("form", list(tc.FORMS))
@pytest.mark.parametrize("name", tc.SHAPES)
def test_crafted_tree_in_every_scoring_form(pmx, oracle, ctx, monkeypatch, name, form):
    _set_form(monkeypatch, form)
    placer = pmx.Placer(ctx, _index(pmx, name))
    assert placer.score_info()["form"] is None
    _score_and_check(pmx, placer, name, form)
    placer.close()


@pytest.mark.parametrize("hist", ["A", "T"])
@pytest.mark.parametrize("name", ["binary", "broom", "random"])
def test_force_leaf_and_bulk_ties(pmx, oracle, ctx, name, hist):
    """the host's two-pass best / tie rule: histogram T makes whole families of nodes share the best score, with forceLeaf only
    leaves may win or tie"""
    placer = pmx.Placer(ctx, _index(pmx, name))
    _, want, _ = _score_and_check(pmx, placer, name, "default", hist, pmx.TraversalParams(forceLeaf=True))
    has_child = np.zeros(tc.tree(name).n_nodes, bool)
    has_child[tc.tree(name).parent[1:]] = True
    assert all(not has_child[t].any() for t in want["ties"])
    if hist == "T":
        assert max(len(t) for t in want["ties"]) > 1
        _, want, _ = _score_and_check(pmx, placer, name, "default", hist)
        assert max(len(t) for t in want["ties"]) > 1
    placer.close()


@pytest.mark.parametrize("name", ["path", "star", "caterpillar"])
def test_bulk_ties_on_deep_and_wide_trees(pmx, oracle, ctx, name):
    placer = pmx.Placer(ctx, _index(pmx, name))
    _, want, _ = _score_and_check(pmx, placer, name, "default", "T")
    assert max(len(t) for t in want["ties"]) > 1
    placer.close()


def test_read_side_edges(pmx, oracle, ctx):
    """seedMaskFraction; a minReadSupport no seed reaches (n_kept == 0, every score 0, the host's "never improved" branch);
    an empty histogram"""
    placer = pmx.Placer(ctx, _index(pmx, "random"))
    _, want, _ = _score_and_check(pmx, placer, "random", "default", "A", pmx.TraversalParams(seedMaskFraction=0.01))
    assert want["state"].n_kept < tc.want("random")["state"].n_kept
    for hist, params in (("low", pmx.TraversalParams(minReadSupport=1000)), ("empty", pmx.TraversalParams())):
        res, want, _ = _score_and_check(pmx, placer, "random", "default", hist, params)
        assert res.readUniqueSeedCount == 0 and not want["scores"].any()
        sc, _, _ = placer.node_outputs()
        assert not sc.any()
        assert all(len(t) == 0 for t in res.tied_indices)
    _score_and_check(pmx, placer, "random", "default", "A")        # and the placer scores a real histogram again
    placer.close()


@pytest.mark.parametrize("levels", [False, True])
@pytest.mark.parametrize("name", ["caterpillar", "random"])
def test_one_placer_across_calls(pmx, oracle, ctx, monkeypatch, name, levels):
    """one placer scored five times: the flags of the persistent kernels are reused by epoch, the status word is cleared after
    a redo, the buffers sized by the histogram move, and the captured level graph is replayed"""
    base = "level_graph" if levels else "default"
    placer = pmx.Placer(ctx, _index(pmx, name))
    for hist, starved in (("A", False), ("B", False), ("A", True), ("A", False), ("C", False)):
        _set_form(monkeypatch, base)
        if starved:
            monkeypatch.setenv("PMX_PLACE_TEST_STARVED", "1")
        # (the level kernels have no persistent launch to starve: the switch is without effect there)
        _score_and_check(pmx, placer, name, "starved" if starved and not levels else base, hist)
    placer.close()
