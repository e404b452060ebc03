"""Score landscapes for the select and replay parity tests (test_landscapes_host.py pins them on the oracle alone;
test_gpu_select_landscapes.py and test_gpu_large_capacity.py run them on the device).

On a cluster of identical empty nodes every pod's plugin total is the same on every node, so a per-pod node score
offset table (an exact integer added to a pair's total) dictates the whole landscape a select sees: where the best
score sits, how many nodes tie with it, how far below the next level lies.  The builders here return (tables, ids)
for node_scores_load / schedule(node_scores=...); the reference stays the lock-step one of test_node_scores_host.py.

Nothing here is imported from the library's dispatch: select_parts and select_boundaries restate the host arithmetic
of the select's wave segments and parts (select_seg / select_part / select_parts in koordinator_amd/csrc/ke_plan.h) in
Python; test_plan_host.py pins them to that header."""
import ctypes as C

import numpy as np

from koordinator_amd import abi, synth
from oracle.binding import Oracle

T0 = synth.T0
SELECT_WAVES = 16   # waves of one select workgroup
STEP = 512          # nodes one wave reads per step (8 scores per lane)
RESIDENT_SEG = 4096  # a wave's segment above this is streamed, not held in registers
WINDOW = 64         # the select's histogram window below the best score
CHG_LDS_NODES = 811_008  # node ids below this fit the replay's LDS changed-node bitmap

HOT_NODES = (137, 400, 9, 555, 64, 63, 512, 511)
HOT_OFFSETS = tuple(range(600, 179, -60))  # 600, 540, ..., 180


# ---- clusters and queues ---------------------------------------------------------------------------------------------
def flat_cluster(n, seed=synth.BASE_SEED + 9401):
    """n identical empty nodes: 64 cores / 256 GiB, no custom thresholds, no NodeMetric, no pods.  Every pod of
    make_pods is feasible everywhere with one total (90..100) on all nodes."""
    cl = synth.make_cluster(n, seed, max_pods_per_node=0)
    cl.nodes[:] = cl.nodes[0]
    cl.nodes["allocatable"][:, 0] = 64 * 1000
    cl.nodes["allocatable"][:, 1] = 256 * synth.GI
    cl.nodes["has_custom_thresholds"] = 0
    for f in ("custom_usage_thresholds", "custom_prod_usage_thresholds", "custom_agg_thresholds"):
        cl.nodes[f][:] = abi.ABSENT
    cl.nm[:] = cl.nm[0]
    cl.has_nm[:] = False
    return cl


def ls_pods(n, seed):
    """n LS pods requesting at least two cores out of make_pods: each Reserve lowers its node's score for every later
    pod on a flat cluster.  (A koord-batch pod leaves it unchanged there, and one core of 64 is 1.6 %, which the integer
    plugin scores of some later pods round away: with one-core pods a later pod returned to a touched node.)"""
    pods = synth.make_pods(4 * n + 64, seed)
    keep = (pods["qos_class"] == abi.QOS_LS) & (pods["requests"][:, abi.RES_CPU] >= 2000) & (pods["is_daemonset"] == 0)
    pods = pods[keep][:n].copy()
    assert len(pods) == n
    return pods


def load_sparse(handle, cl, ids):
    """Node k of `cl` at index ids[k] of an Evaluator or an Oracle, by the per-node informer calls."""
    ids = np.asarray(ids, np.int64)
    for k, i in enumerate(ids):
        i = int(i)
        handle.upsert_node(i, abi.Node.from_buffer_copy(cl.nodes[k:k + 1].tobytes()))
        if cl.has_nm[k]:
            p0, p1 = int(cl.pm_offsets[k]), int(cl.pm_offsets[k + 1])
            a0, a1 = int(cl.agg_offsets[k]), int(cl.agg_offsets[k + 1])
            pm = C.c_void_p(cl.pod_metrics.ctypes.data + p0 * abi.POD_METRIC_DTYPE.itemsize) if p1 > p0 else None
            ag = C.c_void_p(cl.aggregated.ctypes.data + a0 * abi.AGG_DTYPE.itemsize) if a1 > a0 else None
            handle.set_nodemetric(i, (abi.NodeMetric.from_buffer_copy(cl.nm[k:k + 1].tobytes()), pm, p1 - p0, ag, a1 - a0))
    handle.assign_bulk(ids[cl.asg_nodes].astype(np.int32), cl.asg_pods, cl.asg_ts)


def sparse_ids(n_low=300, n_high=300, high=CHG_LDS_NODES):
    """[0, n_low) and [high, high + n_high): the second range lies above the LDS bitmap's node ids."""
    return np.concatenate([np.arange(n_low), high + np.arange(n_high)]).astype(np.int64)


def compact_reference(cfg, cl, ids, pods, now=T0):
    """A sparsely populated index space (node k of `cl` at the increasing index ids[k]): the oracle over the populated
    nodes alone, in index order, with its placements mapped back to the sparse indices.  Unpopulated indices hold no
    node, and increasing ids keep the lowest-index tie-break, so this is the sparse schedule."""
    ids = np.asarray(ids, np.int64)
    assert (np.diff(ids) > 0).all()
    o = Oracle(cfg, cl.n_nodes)
    synth.load_into(o, cl)
    c, s = o.schedule(pods, now)
    return np.where(c >= 0, ids[np.maximum(c, 0)], -1).astype(np.int32), s


# ---- the select's geometry -------------------------------------------------------------------------------------------
def _up(x, m):
    return (x + m - 1) // m * m


def select_parts(n, batch, env=None, list_len=128):
    """Workgroups per pod of a plain batch's select: at least 256 workgroups in all, parts of >= 24576 nodes (4096
    under KOORDEVAL_SELECT_PARTS = env, which also caps them), at most 8, parts x list length <= 1024."""
    cap, per = (8, 24576) if env is None else (max(1, min(8, int(env))), 4096)
    return max(1, min(cap, (255 + batch) // batch, n // per, 1024 // list_len))


def select_boundaries(n, parts=1):
    """The geometry of a select over [0, n) in `parts` parts: a part is ceil(n / parts) rounded up to 512, a wave's
    segment ceil(part range / 16) rounded up to 512, read in steps of 512 nodes.  Returns the part size, per part its
    [lo, hi), segment and the wave starts inside it, the largest segment and whether that one is streamed."""
    part = _up(-(-n // parts), STEP) if parts > 1 else n
    out, seg_max = [], 0
    for p in range(parts):
        lo = min(n, p * part)
        hi = min(n, lo + part)
        seg = _up(-(-(hi - lo) // SELECT_WAVES), STEP)
        waves = [w for w in range(lo, hi, seg)] if hi > lo else []
        out.append(dict(lo=lo, hi=hi, seg=seg, waves=waves))
        seg_max = max(seg_max, seg)
    return dict(part=part, parts=out, seg=seg_max, streamed=seg_max > RESIDENT_SEG)


def boundaries_of(n, parts=1):
    """The three boundaries the tie bands straddle: a 512-node step inside a wave's segment (the first wave's second
    step; with one-step segments that is the second wave's start), a wave-segment boundary (the fourth wave's start)
    and the first part boundary (None with one part)."""
    g = select_boundaries(n, parts)
    p0 = g["parts"][0]
    return dict(step=p0["lo"] + STEP, segment=p0["waves"][3], part=g["parts"][1]["lo"] if parts > 1 else None)


def all_boundaries(n, parts=1):
    """Every wave start and part start of the select inside (0, n)."""
    g = select_boundaries(n, parts)
    return sorted({w for p in g["parts"] for w in p["waves"] if 0 < w < n})


# ---- offset tables ---------------------------------------------------------------------------------------------------
def _one(table, n_pods):
    return table[None, :], np.ones(n_pods, np.int32)


def tie_band(n, start, n_pods, width=400, value=100):
    """+value on the `width` nodes from `start`: every pod's best score ties on the band's untouched nodes."""
    t = np.zeros(n, np.int64)
    assert 0 <= start and start + width <= n
    t[start:start + width] = value
    return _one(t, n_pods)


def band_start(n, parts, which):
    """Where the 400-node band of a tie-band case starts: 20 nodes before its boundary, or at n - 400 ("tail")."""
    return n - 400 if which == "tail" else boundaries_of(n, parts)[which] - 20


def sparse_top(n, parts, n_pods, top=500, second=470, level=400):
    """+500 on 5 scattered nodes, +470 on 3, +400 on 200, 0 elsewhere: fewer than k nodes lie within the window of
    the best score (the gap of 70 exceeds it), and the 200-node level forces a tie cut below it.  The scattered nodes
    sit on both sides of wave and part boundaries and at both ends; the level straddles a segment boundary.
    (No Reserve lowers a total by 100, so the pods stay on the eight nodes: the cut is computed and never consumed.
    "sparse-near" is the same shape at 170 / 165 / 100 under the LS queue: the eight nodes sink below the level while
    the queue runs, so pods take the level's nodes in index order -- the entries the search's tie cut admitted.)"""
    b = all_boundaries(n, parts)
    t = np.zeros(n, np.int64)
    seg = boundaries_of(n, parts)["segment"]
    at = (np.arange(200) * 3 + seg - 150) % n  # every third node across the segment boundary
    t[at] = level
    t[[n - 1, b[-1], b[len(b) // 2] - 1]] = second
    t[[0, b[0] - 1, b[0], b[len(b) // 2], n - 2]] = top
    assert (t == top).sum() == 5 and (t == second).sum() == 3 and 192 <= (t == level).sum() <= 200
    return _one(t, n_pods)


def window_edge(n, parts, n_pods, variant, top=600):
    """One node at each of top, top - 1, ..., top - 63 at descending node indices (score order is the reverse of the
    index order) and a plateau of 300 nodes at top - 63 (variant 1: the cut falls in the window's last bin) or at
    top - 64 (variant 2: just outside the window).  (The pods stay on the first 30 single nodes: the landscape checks
    that the threshold at the window's edge yields lists the replay can use, not which plateau node a cut admits --
    the tie bands and "sparse-near" consume their cuts.)"""
    t = np.zeros(n, np.int64)
    seg = boundaries_of(n, parts)["segment"]
    stride = (n - 1) // WINDOW
    singles = (n - 1) - np.arange(WINDOW) * stride
    plateau = np.setdiff1d(np.arange(seg - 20, seg + 400), singles)[:300]  # 300 nodes across a segment boundary
    t[plateau] = top - (63 if variant == 1 else 64)
    t[singles] = top - np.arange(WINDOW)
    return _one(t, n_pods)


FEW_SIZES = (10, 64, 65, 200)


def few_feasible(n, parts, n_pods):
    """Node sets that leave exactly 10, 64, 65 and 200 eligible nodes -- node 0, node n - 1 and both neighbours of
    every wave and part boundary first, then evenly spread ones -- and the set id per pod: batch positions 8, 9 and
    20 take the 10-node set (F == k + 1, F == k, F < k with exact lists), 62 and 63 the 64- and 65-node sets
    (F == k + 1 twice), the others cycle through all four."""
    must = [0, n - 1]
    part_starts = [p["lo"] for p in select_boundaries(n, parts)["parts"][1:]]
    for b in part_starts + all_boundaries(n, parts):  # (the part boundaries first: the 10-node set holds them too)
        must += [b - 1, b]
    sets = np.zeros((len(FEW_SIZES), n), bool)
    for s, size in enumerate(FEW_SIZES):
        pick = list(dict.fromkeys(must))[:size]  # (the small sets hold the first boundaries' neighbours only)
        have = set(pick)
        fill = [int(x) for x in np.linspace(1, n - 2, 4 * size).astype(np.int64) if int(x) not in have]
        pick = (pick + fill)[:size]
        sets[s, pick] = True
        assert sets[s].sum() == size
    pos = np.arange(n_pods) % 64
    sids = 1 + np.arange(n_pods) % len(FEW_SIZES)
    sids[(pos == 8) | (pos == 9) | (pos == 20)] = 1
    sids[pos == 62] = 2
    sids[pos == 63] = 3
    return sets, sids.astype(np.int32)


def hot_nodes(n, n_pods):
    """600, 540, ..., 180 on eight nodes of a synthetic cluster: pods crowd onto the same few nodes until they fill,
    so a batch's pods choose nodes that earlier pods of the batch, and the previous batch, changed."""
    t = np.zeros(n, np.int64)
    t[list(HOT_NODES)] = HOT_OFFSETS
    return _one(t, n_pods)


def repeat_counts(chosen, batch=64):
    """(pods that chose a node an earlier pod of their batch chose, pods that chose a node the previous batch chose,
    placed pods) of a placement vector."""
    in_batch = prev_batch = 0
    prev = set()
    for a in range(0, len(chosen), batch):
        seen = set()
        for c in chosen[a:a + batch]:
            c = int(c)
            if c < 0:
                continue
            in_batch += c in seen
            prev_batch += c in prev
            seen.add(c)
        prev = seen
    return in_batch, prev_batch, int((np.asarray(chosen) >= 0).sum())


# ---- the cases of the select tests: a landscape on a flat cluster in one select configuration ---------------------------
# id -> (nodes, KOORDEVAL_SELECT_PARTS or None, parts a 64-pod batch's select then runs in)
CONFIGS = {"one-part": (8_200, None, 1), "split": (8_200, "8", 2), "stream": (66_061, "1", 1),
           "stream-split": (140_003, "2", 2)}
TIE_LANDSCAPES = ("all-tie", "band-step", "band-segment", "band-part", "band-tail", "sparse-near")
LANDSCAPES = TIE_LANDSCAPES + ("sparse-top", "window-edge-1", "window-edge-2", "few-feasible")
N_PODS = 192
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def landscape(name, n, parts):
    """The inputs of landscape `name` over n flat nodes selected in `parts` parts: cluster, queue, offset tables with
    the table id per pod (or None), node sets with the set id per pod (or None), the band's first node (or None)."""
    cl = cached(("flat", n), lambda: flat_cluster(n))
    pods = (ls_pods(N_PODS, synth.BASE_SEED + 9403) if name in TIE_LANDSCAPES
            else synth.make_pods(N_PODS, synth.BASE_SEED + 9402))
    tables = ids = sets = sids = start = None
    if name.startswith("band-"):
        start = band_start(n, parts, name[5:])
        tables, ids = tie_band(n, start, N_PODS)
    elif name == "sparse-top":
        tables, ids = sparse_top(n, parts, N_PODS)
    elif name == "sparse-near":
        tables, ids = sparse_top(n, parts, N_PODS, 170, 165, 100)
    elif name.startswith("window-edge-"):
        tables, ids = window_edge(n, parts, N_PODS, int(name[-1]))
    elif name == "few-feasible":
        sets, sids = few_feasible(n, parts, N_PODS)
    else:
        assert name == "all-tie", name
    return dict(n=n, cl=cl, pods=pods, tables=tables, ids=ids, sets=sets, sids=sids, start=start)


def landscape_reference(name, n, parts):
    """landscape() with `want`: the lock-step reference with the case's offsets and sets (the oracle's own schedule
    when it has neither), computed once."""
    from test_node_scores_host import lockstep_scores, offsets_of

    def make():
        c = landscape(name, n, parts)
        o = Oracle(synth.config(n), n)
        synth.load_into(o, c["cl"])
        if c["tables"] is None and c["sets"] is None:
            c["want"] = o.schedule(c["pods"], T0)
        else:
            off = offsets_of(c["tables"] if c["tables"] is not None else [], c["ids"] if c["ids"] is not None
                             else np.zeros(N_PODS, np.int32), n)
            elig = None if c["sets"] is None else c["sets"][c["sids"] - 1]
            c["want"] = lockstep_scores(o, c["pods"], off, elig)
        return c
    return cached(("ref", name, n, parts), make)
