"""The references and inputs of the select-landscape and large-capacity GPU tests (landscapes.py), pinned on the
oracle alone: the flat cluster is flat, the compact reference of a sparsely populated index space is the sparse
oracle's schedule, and each landscape has the property its GPU cases rely on -- computed from the reference
placements.  These are conditions on the inputs: a queue or a table that misses one is replaced, not the bound."""
import numpy as np
import pytest

import landscapes as L
from koordinator_amd import synth
from oracle.binding import Oracle
from test_node_scores_host import lockstep_scores, offsets_of

T0 = synth.T0


def test_flat_cluster_is_flat():
    n = 600
    o = Oracle(synth.config(n), n)
    synth.load_into(o, L.flat_cluster(n))
    for pods in (synth.make_pods(L.N_PODS, synth.BASE_SEED + 9402), L.ls_pods(L.N_PODS, synth.BASE_SEED + 9403)):
        r = o.eval(pods, T0)
        assert (r["status"] == 0).all()
        assert (r["total"].max(1) == r["total"].min(1)).all()
        assert 90 <= r["total"].min() and r["total"].max() <= 100


def test_select_boundaries_restate_the_dispatch():
    """Segments and parts of the four select configurations, by hand: 8,200 nodes in one part give 16 segments of
    ceil(8200 / 16) = 513 -> 1024 nodes (two steps each); in two parts of 4100 -> 4608 nodes, segments of 288 -> 512;
    66,061 nodes in one part give 4129 -> 4608 > 4096 (streamed); 140,003 in two parts of 70,002 -> 70,144 give
    4384 -> 4608 (streamed)."""
    want = {"one-part": (8_200, 1024, False), "split": (4_608, 512, False), "stream": (66_061, 4_608, True),
            "stream-split": (70_144, 4_608, True)}
    for name, (n, env, parts) in L.CONFIGS.items():
        g = L.select_boundaries(n, parts)
        assert (g["part"], g["seg"], g["streamed"]) == want[name], name
        # the dispatch's part count for 64-pod batches and every list length it uses (serial 64, stale 128, ahead 192)
        for ll in (64, 128, 192):
            assert L.select_parts(n, 64, env, ll) == parts, (name, ll)
        assert g["parts"][-1]["hi"] == n and all(p["hi"] > p["lo"] for p in g["parts"])
    assert n % 8 != 0 and L.CONFIGS["stream"][0] % 8 != 0  # a last 16-byte load that is partial
    # the sparse high-id run: four parts of about 200k nodes, streamed
    n = L.CHG_LDS_NODES + 300
    assert L.select_parts(n, 64) == 4
    g = L.select_boundaries(n, 4)
    assert g["streamed"] and g["part"] == 203_264


def test_compact_reference_is_the_sparse_schedule():
    cl = synth.make_cluster(600, synth.BASE_SEED + 5)
    pods = synth.make_pods(24, synth.BASE_SEED + 6)
    ids = L.sparse_ids()
    n = int(ids[-1]) + 1
    assert n == 811_308
    o = Oracle(synth.config(n), n)
    L.load_sparse(o, cl, ids)
    c0, s0 = o.schedule(pods, T0)
    c1, s1 = L.compact_reference(synth.config(600), cl, ids, pods)
    assert np.array_equal(c0, c1) and np.array_equal(s0, s1)
    assert (c0 >= 0).all() and (c0 >= L.CHG_LDS_NODES).any() and (c0 < 300).any()


def test_sparse_high_ids_are_chosen():
    cl = synth.make_cluster(600, synth.BASE_SEED + 5)
    c, _ = L.compact_reference(synth.config(600), cl, L.sparse_ids(), synth.make_pods(200, synth.BASE_SEED + 6))
    assert int((c >= L.CHG_LDS_NODES).sum()) >= 20
    assert int(((c >= 0) & (c < 300)).sum()) >= 20


@pytest.mark.parametrize("n_pods", [256, 384])
def test_hot_nodes_repeat_within_and_across_batches(n_pods):
    n = 600
    cl = synth.make_cluster(n, synth.BASE_SEED + 5)
    pods = synth.make_pods(n_pods, synth.BASE_SEED + 6)
    o = Oracle(synth.config(n), n)
    synth.load_into(o, cl)
    tables, ids = L.hot_nodes(n, n_pods)
    c, _ = lockstep_scores(o, pods, offsets_of(tables, ids, n))
    in_batch, prev_batch, placed = L.repeat_counts(c, 64)
    assert placed == n_pods
    assert 5 * in_batch >= placed, (in_batch, placed)
    assert prev_batch >= 20, prev_batch
    if n_pods == 384:
        assert in_batch == 82


@pytest.mark.parametrize("config,which", [(c, w) for c in ("one-part", "split") for w in ("step", "segment", "part", "tail")
                                          if w != "part" or L.CONFIGS[c][2] > 1])
def test_tie_band_is_consumed_in_index_order(config, which):
    """Serial mode's exact lists hold k_j = j + 1 entries: pod j of a batch needs the j-th untouched band node, the
    last entry of its list.  (The band's geometry at the two large node counts is the same arithmetic; their GPU cases
    assert the same condition on their own reference.)"""
    n, _, parts = L.CONFIGS[config]
    c = L.landscape_reference("band-" + which, n, parts)
    assert_band_consumed(c, n, parts, which)


def assert_band_consumed(c, n, parts, which):
    chosen, start = c["want"][0], c["start"]
    for a in range(0, len(chosen), 64):  # pod j of the batch: the j-th lowest untouched band node
        untouched = np.setdiff1d(np.arange(start, start + 400), chosen[:a])
        assert np.array_equal(chosen[a:a + 64], untouched[:len(chosen[a:a + 64])]), a
    if which != "tail":
        b = L.boundaries_of(n, parts)[which]
        assert int((chosen < b).sum()) >= 10 and int((chosen >= b).sum()) >= 10
    else:
        assert start + 400 == n


@pytest.mark.parametrize("config", ["one-part", "split"])
def test_sparse_near_consumes_the_level(config):
    """The eight top nodes sink below the 200-node level while the queue runs: at least 20 pods are placed on top
    nodes while the level lies outside the window, and at least 20 take the level's nodes, lowest index first."""
    n, _, parts = L.CONFIGS[config]
    c = L.landscape_reference("sparse-near", n, parts)
    lv = c["tables"][0][c["want"][0]]
    assert int((lv >= 165).sum()) >= 20 and int((lv == 100).sum()) >= 20 and int((lv == 0).sum()) == 0
    took = c["want"][0][lv == 100]
    assert (np.diff(took) > 0).all()


def test_threshold_landscapes_have_their_levels():
    n, _, parts = L.CONFIGS["one-part"]
    t = L.sparse_top(n, parts, 4)[0][0]
    levels = np.unique(t)[::-1]
    assert levels[0] - levels[1] < L.WINDOW and levels[1] - levels[2] > L.WINDOW  # 500, 470 | 400: outside the window
    assert (t >= levels[1]).sum() == 8  # k > 8 finds fewer than k nodes inside the window
    for variant, gap in ((1, 63), (2, 64)):
        t = L.window_edge(n, parts, 4, variant)[0][0]
        top = int(t.max())
        singles = np.array([int(np.nonzero(t == top - i)[0].min()) for i in range(L.WINDOW - (variant == 1))])
        assert (np.diff(singles) < 0).all()  # score order is the reverse of index order
        assert (t == top - gap).sum() == 300 + (variant == 1) and ((t > top - gap) & (t > 0)).sum() == (63 if variant == 1 else 64)
    sets, sids = L.few_feasible(n, parts, L.N_PODS)
    assert sets.sum(1).tolist() == list(L.FEW_SIZES) and sets[:, 0].all() and sets[:, n - 1].all()
    for b in L.all_boundaries(n, parts):
        assert sets[1:, b - 1].all() and sets[1:, b].all(), b
    assert sids[8] == sids[9] == 1 and sids[62] == 2 and sids[63] == 3
