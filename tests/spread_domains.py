"""Inputs and the lock-step reference of the spread domain tests (test_spread_domains_host.py pins them on the oracle
alone; test_gpu_spread_domains.py runs them on the device).

A spread domain group g has a domain map, a `domains` bitmask, maxSkew, minDomains and a pod count per domain; node n
with domain d = map[n] is filtered for the group's pods when d is NONE, outside `domains`, or
count[g][d] + 1 - min > maxSkew (min over `domains`, 0 when they are fewer than minDomains), and every placement
increments its domain's count.  The reference is the spread groups' lock-step oracle with that one
more piece of state: per pod the oracle's eval total (+ the pod's score offset), masked with (node set), (§4r count
below its cap) and (domain open), selectHost's argmax, the Reserve by hand, the increments.
"""
import numpy as np

from koordinator_amd import abi, synth
from landscapes import HOT_NODES, HOT_OFFSETS
from oracle.binding import Oracle
from test_node_sets_host import manual_reserve, masked_argmax

T0 = synth.T0
N_PODS = 256
WINDOW = 64  # the window the "moved" / "newly eligible" statistics refer to: what an uncut 64-pod batch would see
NONE = abi.DOMAIN_NONE
D = abi.MAX_SPREAD_DOMAINS

# id -> (nodes, seed - BASE_SEED, grouped fraction, highest seed count)
INPUTS = {"E": (333, 9748, 0.75, 2), "F": (333, 9710, 1.0, 2), "G": (130, 9720, 1.0, 2), "H": (600, 9730, 1.0, 0)}
_CACHE = {}


def full_mask(d):
    """The `domains` bitmask of domains 0 .. d-1."""
    return (1 << d) - 1


def _maps_and_groups(name, n, rng):
    """(maps [M, n] of domain ids, groups as (map 1-based, domains mask, maxSkew, minDomains))."""
    if name == "E":  # a zone map of 3 domains of uneven sizes, a rack map of 7
        zone = rng.choice(3, n, p=(0.55, 0.3, 0.15))
        rack = rng.integers(0, 7, n)
        return np.stack([zone, rack]), [(1, full_mask(3), 1, 0), (1, full_mask(3), 2, 0), (2, full_mask(7), 1, 0)]
    if name == "F":  # zone = node mod 3; a 64-domain map, some of its domains without a node
        m64 = rng.choice(np.setdiff1d(np.arange(64), [5, 17, 40, 63]), n)
        return np.stack([np.arange(n) % 3, m64]), [(1, full_mask(3), 1, 0), (2, full_mask(64), 1, 0)]
    if name == "G":  # 5 domains; the second group asks for 8, so its minimum is 0
        return rng.integers(0, 5, (1, n)), [(1, full_mask(5), 1, 0), (1, full_mask(5), 1, 8)]
    if name == "H":  # a 1-domain map (always open: the minimum is its own count) and a map of 4 blocks
        return np.stack([np.zeros(n, np.int64), np.arange(n) * 4 // n]), [(1, 1, 1, 0), (2, full_mask(4), 2, 0),
                                                                          (2, full_mask(4), 1, 0)]
    raise KeyError(name)


def make_input(name, extras=False):
    """dict(n, cl, pods, maps [M, n] uint16, gmap / dom / skew / mind [G], dids [P], dcounts [G, 64] uint32, and --
    with `extras`: input-D style spread groups (zero seeds), node sets and a score table besides -- caps, counts, gids,
    sets, sids, table, tids (else None))."""
    if ("in", name, extras) in _CACHE:
        return _CACHE[("in", name, extras)]
    n, seed, frac, top = INPUTS[name]
    seed += synth.BASE_SEED
    cl = synth.make_cluster(n, seed)
    pods = synth.make_pods(N_PODS, seed + 1)
    rng = np.random.default_rng(seed + 2)
    maps, groups = _maps_and_groups(name, n, rng)
    maps = maps.astype(np.int64)
    maps[:, rng.random(n) < 0.05] = NONE  # nodes without the topology keys
    G = len(groups)
    dids = np.where(rng.random(N_PODS) < frac, rng.integers(1, G + 1, N_PODS), 0).astype(np.int32)
    dcounts = np.zeros((G, D), np.uint32)
    for g, (_, mask, _, _) in enumerate(groups):
        for d in range(D):
            if (mask >> d) & 1:
                dcounts[g, d] = rng.integers(0, top + 1)
    c = dict(n=n, cl=cl, pods=pods, maps=maps.astype(np.uint16), gmap=np.array([g[0] for g in groups], np.int32),
             dom=[g[1] for g in groups], skew=np.array([g[2] for g in groups], np.int32),
             mind=np.array([g[3] for g in groups], np.int32), dids=dids, dcounts=dcounts,
             caps=None, counts=None, gids=None, sets=None, sids=None, table=None, tids=None)
    if extras:
        xr = np.random.default_rng(seed + 3)
        sets = xr.random((2, n)) < 0.5
        hot = [(h, o) for h, o in zip(HOT_NODES, HOT_OFFSETS) if h < n]  # (the landscape's hot nodes this cluster has)
        sets[:, [h for h, _ in hot]] = True
        table = np.zeros(n, np.int64)
        table[[h for h, _ in hot]] = [o for _, o in hot]
        c.update(caps=np.array([1, 2, 2], np.uint16), counts=np.zeros((3, n), np.uint16),
                 gids=xr.integers(1, 4, N_PODS).astype(np.int32), sets=sets, sids=xr.integers(0, 3, N_PODS).astype(np.int32),
                 table=table, tids=np.ones(N_PODS, np.int32))
    _CACHE[("in", name, extras)] = c
    return c


def eligibility(c):
    """bool [pod, node] of the pods' node sets (every node without sets)."""
    if c["sets"] is None:
        return np.ones((len(c["pods"]), c["n"]), bool)
    return np.concatenate([np.ones((1, c["n"]), bool), c["sets"]])[c["sids"]]


def offsets(c):
    """int64 [pod, node] score offsets (zero without a table)."""
    if c["table"] is None:
        return np.zeros((len(c["pods"]), c["n"]), np.int64)
    return np.concatenate([np.zeros((1, c["n"]), np.int64), c["table"][None]])[c["tids"]]


def group_ids(c):
    return np.zeros(len(c["pods"]), np.int32) if c["gids"] is None else c["gids"]


def fresh_oracle(c):
    o = Oracle(synth.config(c["n"]), c["n"])
    synth.load_into(o, c["cl"])
    return o


def open_domains(dom, skew, mind, counts):
    """bool [64]: the domains open to a pod of a group with these parameters and counts [64] (upstream's Filter)."""
    inside = np.array([(int(dom) >> d) & 1 for d in range(D)], bool)
    least = 0 if int(inside.sum()) < int(mind) else int(counts[inside].min())
    return inside & (counts.astype(np.int64) + 1 - least <= int(skew))


class Lockstep:
    """The reference's state: an oracle, the domain counts [G + 1, 64] (row 0 unused) and the §4r counts [S + 1, n]
    (row 0 stays zero; caps[0] is never reached)."""

    def __init__(self, o, c):
        self.o, self.n = o, c["n"]
        self.maps = np.concatenate([np.zeros((1, c["n"]), np.int64), c["maps"].astype(np.int64)])
        self.gmap = np.concatenate([[0], c["gmap"]])
        self.dom, self.skew, self.mind = [0] + list(c["dom"]), np.concatenate([[0], c["skew"]]), np.concatenate([[0], c["mind"]])
        self.dcounts = np.concatenate([np.zeros((1, D), np.int64), c["dcounts"].astype(np.int64)])
        sg = np.zeros((0, c["n"]), np.int64) if c["counts"] is None else c["counts"].astype(np.int64)
        self.counts = np.concatenate([np.zeros((1, c["n"]), np.int64), sg])
        self.caps = np.concatenate([[1 << 30], [] if c["caps"] is None else np.asarray(c["caps"], np.int64)]).astype(np.int64)

    def domain_ok(self, did, dcounts=None):
        """bool [node]: the nodes whose domain is open to a pod of spread domain group `did` (0: every node)."""
        if did == 0:
            return np.ones(self.n, bool)
        d = self.maps[self.gmap[did]]
        op = open_domains(self.dom[did], self.skew[did], self.mind[did], (self.dcounts if dcounts is None else dcounts)[did])
        return (d < D) & op[np.minimum(d, D - 1)]

    def step(self, pod, did, gid, elig, off, stale=None):
        """Place one pod; returns (node, score, the best node by the node set and cap alone or -1, the node the pod
        would have taken had the domain counts been `stale` -- None: not asked for)."""
        total = self.o.eval(pod.reshape(1), T0)["total"][0].astype(np.int64)
        total = np.where(total >= 0, total + off, -1)
        base = elig & (self.counts[gid] < self.caps[gid])
        free, _ = masked_argmax(total, base)
        old = None if stale is None else masked_argmax(total, base & self.domain_ok(did, stale))[0]
        node, score = masked_argmax(total, base & self.domain_ok(did))
        if node >= 0:
            manual_reserve(self.o, node, pod)
            self.counts[gid, node] += gid > 0
            if did:
                self.dcounts[did, self.maps[self.gmap[did], node]] += 1
        return node, score, free, old

    def run(self, pods, dids, gids, elig, off):
        chosen, score = np.full(len(pods), -1, np.int32), np.full(len(pods), -1, np.int32)
        for p in range(len(pods)):
            chosen[p], score[p] = self.step(pods[p], int(dids[p]), int(gids[p]), elig[p], off[p])[:2]
        return chosen, score


def reference(name, extras=False):
    """make_input(name) with the lock-step result, computed once: want = (chosen, score), dcounts_after [G, 64],
    counts_after (§4r, or None), and the statistics that keep the GPU tests from passing vacuously -- best_filtered:
    pods whose best node by set and cap alone was closed by the skew when they were placed; moved: pods that would have
    gone elsewhere had they seen the domain counts as they stood at the start of their 64-pod window (what an uncut
    batch computes); newly: pods that landed on a node closed to them at the start of their window; unplaced; and
    skew_ok: every placement satisfied the skew bound when it was made."""
    if ("ref", name, extras) in _CACHE:
        return _CACHE[("ref", name, extras)]
    c = dict(make_input(name, extras))
    ls = Lockstep(fresh_oracle(c), c)
    elig, off, gids = eligibility(c), offsets(c), group_ids(c)
    P = len(c["pods"])
    chosen, score = np.full(P, -1, np.int32), np.full(P, -1, np.int32)
    best_filtered = moved = newly = 0
    skew_ok = True
    for p in range(P):
        if p % WINDOW == 0:
            at_start = ls.dcounts.copy()
        did = int(c["dids"][p])
        ok_now, ok_then = ls.domain_ok(did), ls.domain_ok(did, at_start)
        before = ls.dcounts[did].copy()
        chosen[p], score[p], free, old = ls.step(c["pods"][p], did, int(gids[p]), elig[p], off[p], stale=at_start)
        best_filtered += free >= 0 and not ok_now[free]
        moved += old != chosen[p]
        newly += chosen[p] >= 0 and not ok_then[chosen[p]]
        if did and chosen[p] >= 0:
            d = int(ls.maps[ls.gmap[did], chosen[p]])
            inside = np.array([(int(ls.dom[did]) >> q) & 1 for q in range(D)], bool)
            least = 0 if inside.sum() < ls.mind[did] else before[inside].min()
            skew_ok = skew_ok and d < D and bool(inside[d]) and before[d] + 1 - least <= ls.skew[did]
    c.update(want=(chosen, score), dcounts_after=ls.dcounts[1:].astype(np.uint32),
             counts_after=None if c["counts"] is None else ls.counts[1:].astype(np.uint16), best_filtered=int(best_filtered),
             moved=int(moved), newly=int(newly), unplaced=int((chosen < 0).sum()), skew_ok=bool(skew_ok))
    _CACHE[("ref", name, extras)] = c
    return c


def reference_without_domains(name, extras=False):
    """The same run with every spread domain id 0 (spread groups, node sets and offsets kept): (chosen, score)."""
    if ("nodomains", name, extras) not in _CACHE:
        c = make_input(name, extras)
        ls = Lockstep(fresh_oracle(c), c)
        _CACHE[("nodomains", name, extras)] = ls.run(c["pods"], np.zeros(len(c["pods"]), np.int32), group_ids(c),
                                                     eligibility(c), offsets(c))
    return _CACHE[("nodomains", name, extras)]


def plan(dids, batch):
    """ke_plan.h's segmentation of a plain queue restated: the pod count of every batch -- up to `batch` pods, ended
    before a pod whose non-zero id already occurs in the batch."""
    out, seen, cur = [], set(), 0
    for d in dids:
        d = int(d)
        if cur == batch or (d and d in seen):
            out.append(cur)
            seen, cur = set(), 0
        cur += 1
        if d:
            seen.add(d)
    return out + [cur] if cur else out


def load(ev, c):
    """The input's tables into an Evaluator; returns the keyword arguments of its schedule / submit / eval calls."""
    ev.spread_domains_load(c["maps"], c["gmap"], c["dom"], c["skew"], c["mind"], c["dcounts"])
    kw = dict(spread_domains=c["dids"])
    if c["sets"] is not None:
        ev.spread_groups_load(c["counts"], c["caps"])
        ev.node_sets_load(c["sets"])
        ev.node_scores_load(c["table"][None])
        kw.update(spread_groups=c["gids"], node_sets=c["sids"], node_scores=c["tids"])
    return kw


def slice_kw(kw, a, b):
    return {k: v[a:b] for k, v in kw.items()}
