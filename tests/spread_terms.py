"""Inputs and the lock-step reference of the spread term tests (test_spread_terms_host.py pins them on the oracle
alone; test_gpu_spread_terms.py runs them on the device).

A pod carries terms over the spread groups' counts -- ANTI (node filtered at count >= param), AFFINITY (filtered at
count < param), PREFER_FEWER / PREFER_MORE (a bonus from the clipped count) -- and members, the groups whose count on
its node a placement increments, saturating at 65535.  The reference is the spread groups' lock-step
oracle with lists: per pod the oracle's eval total (+ the pod's score offset + the bonus), masked with (node set),
(spread domain open) and (every filter term), selectHost's argmax, the Reserve by hand, the members' increments.
"""
import numpy as np

from koordinator_amd import abi, synth
from oracle.binding import Oracle
from spread_domains import Lockstep as DomainLockstep
from spread_domains import make_input as domain_input
from test_node_sets_host import manual_reserve, masked_argmax

T0 = synth.T0
N_PODS = 256
BATCH = 64  # the batch the "depends on its own batch" statistics refer to
ANTI, AFFINITY, FEWER, MORE = abi.TERM_ANTI, abi.TERM_AFFINITY, abi.TERM_PREFER_FEWER, abi.TERM_PREFER_MORE
SAT = 65535

# id -> (nodes, seed - BASE_SEED, groups); X: spread_domains' input E with its node sets, score table and domain ids
INPUTS = {"T": (333, 9810, 4), "U": (333, 9820, 6), "V": (130, 9830, 3), "W": (600, 9840, 5), "X": (333, 9850, 4)}
_CACHE = {}


def draw_lists(rng, n_pods, G):
    """The per-pod lists: every pod is a member of its own group, 30 % of a second one; 40 % carry ANTI on their own
    group (param 1 or 2), 30 % ANTI(…, 1) on another group, 25 % AFFINITY(…, 1) on a partner group; 70 % carry
    PREFER_FEWER on their own group, the others PREFER_MORE on the partner group."""
    terms, members = [], []
    for _ in range(n_pods):
        own = int(rng.integers(1, G + 1))
        other = int(1 + (own - 1 + rng.integers(1, G)) % G)
        partner = int(1 + (own - 1 + rng.integers(1, G)) % G)
        tl, ml = [], [own]
        if rng.random() < 0.4:
            tl.append((own, ANTI, int(rng.integers(1, 3)), 0))
        if rng.random() < 0.3:
            tl.append((other, ANTI, 1, 0))
        if rng.random() < 0.25 and not any(t[0] == partner for t in tl):  # (not ANTI and AFFINITY on one group)
            tl.append((partner, AFFINITY, 1, 0))
        if rng.random() < 0.7:
            tl.append((own, FEWER, int(rng.integers(1, 4)), int(rng.integers(2, 21))))
        else:
            tl.append((partner, MORE, int(rng.integers(1, 4)), int(rng.integers(2, 21))))
        if rng.random() < 0.3:
            ml.append(other)
        terms.append(tl)
        members.append(ml)
    return terms, members


def make_input(name):
    """dict(n, cl, pods, G, counts [G, n] uint16 (about 5 % seeded), terms / members (per-pod lists), and -- input X
    only, else None -- dom (spread_domains' input E with extras: its maps, groups, dids, sets, sids, table, tids))."""
    if ("in", name) in _CACHE:
        return _CACHE[("in", name)]
    n, seed, G = INPUTS[name]
    seed += synth.BASE_SEED
    dom = None
    if name == "X":
        dom = domain_input("E", extras=True)
        assert dom["n"] == n
        cl, pods = dom["cl"], dom["pods"]
    else:
        cl = synth.make_cluster(n, seed)
        pods = synth.make_pods(N_PODS, seed + 1)
    rng = np.random.default_rng(seed + 2)
    counts = (rng.random((G, n)) < 0.05).astype(np.uint16)
    terms, members = draw_lists(rng, N_PODS, G)
    c = dict(n=n, cl=cl, pods=pods, G=G, counts=counts, terms=terms, members=members, dom=dom)
    _CACHE[("in", name)] = c
    return c


def affinity_only_input():
    """Zero seeds and AFFINITY-only pods that are members of another group: nobody can be placed."""
    c = dict(make_input("V"))
    c["counts"] = np.zeros_like(c["counts"])
    c["terms"] = [[(1 + p % c["G"], AFFINITY, 1, 0)] for p in range(N_PODS)]
    c["members"] = [[1 + (p + 1) % c["G"]] for p in range(N_PODS)]
    return c


def eligibility(c):
    """bool [pod, node] of the pods' node sets (every node without sets)."""
    d = c["dom"]
    if d is None:
        return np.ones((len(c["pods"]), c["n"]), bool)
    return np.concatenate([np.ones((1, c["n"]), bool), d["sets"]])[d["sids"]]


def offsets(c):
    """int64 [pod, node] score offsets (zero without a table)."""
    d = c["dom"]
    if d is None:
        return np.zeros((len(c["pods"]), c["n"]), np.int64)
    return np.concatenate([np.zeros((1, c["n"]), np.int64), d["table"][None]])[d["tids"]]


def domain_ids(c):
    return np.zeros(len(c["pods"]), np.int32) if c["dom"] is None else c["dom"]["dids"]


def fresh_oracle(c):
    o = Oracle(synth.config(c["n"]), c["n"])
    synth.load_into(o, c["cl"])
    return o


def apply_terms(terms, counts):
    """(open [n] bool, bonus [n] int64) of a term list against counts [G + 1, n]."""
    n = counts.shape[1]
    ok, bonus = np.ones(n, bool), np.zeros(n, np.int64)
    for g, kind, param, weight in terms:
        cnt = counts[g]
        if kind == ANTI:
            ok &= cnt < param
        elif kind == AFFINITY:
            ok &= cnt >= param
        elif kind == FEWER:
            bonus += weight * (param - np.minimum(cnt, param))
        elif kind == MORE:
            bonus += weight * np.minimum(cnt, param)
        else:
            raise ValueError(kind)
    return ok, bonus


def without_score_terms(terms):
    return [[t for t in tl if t[1] in (ANTI, AFFINITY)] for tl in terms]


class Lockstep:
    """The reference's state: an oracle, the counts [G + 1, n] (row 0 stays zero) and -- with spread domain ids --
    spread_domains' lock-step state for the domain counts."""

    def __init__(self, o, c):
        self.o, self.n = o, c["n"]
        self.counts = np.concatenate([np.zeros((1, c["n"]), np.int64), c["counts"].astype(np.int64)])
        self.dom = None
        if c["dom"] is not None:
            d = dict(c["dom"])
            d.update(counts=None, caps=None)  # (the §4r counts are this class's)
            self.dom = DomainLockstep(None, d)

    def domain_ok(self, did):
        return np.ones(self.n, bool) if self.dom is None else self.dom.domain_ok(did)

    def pick(self, total, off, terms, base, counts):
        """selectHost of one pod with the term lists read against `counts`: (node, score)."""
        ok, bonus = apply_terms(terms, counts)
        return masked_argmax(np.where(total >= 0, total + off + bonus, -1), base & ok)

    def step(self, pod, terms, members, elig, off, did=0, stale=None):
        """Place one pod; returns (node, score, the best node by set, domain and offset alone or -1, the node the pod
        would have taken had the counts been `stale` -- None: not asked for)."""
        total = self.o.eval(pod.reshape(1), T0)["total"][0].astype(np.int64)
        base = elig & self.domain_ok(did)
        free, _ = masked_argmax(np.where(total >= 0, total + off, -1), base)
        old = None if stale is None else self.pick(total, off, terms, base, stale)[0]
        node, score = self.pick(total, off, terms, base, self.counts)
        if node >= 0:
            manual_reserve(self.o, node, pod)
            for m in members:
                self.counts[m, node] = min(self.counts[m, node] + 1, SAT)
            if did:
                self.dom.dcounts[did, self.dom.maps[self.dom.gmap[did], node]] += 1
        return node, score, free, old

    def run(self, pods, terms, members, elig, off, dids=None):
        chosen, score = np.full(len(pods), -1, np.int32), np.full(len(pods), -1, np.int32)
        for p in range(len(pods)):
            chosen[p], score[p] = self.step(pods[p], terms[p], members[p], elig[p], off[p],
                                            0 if dids is None else int(dids[p]))[:2]
        return chosen, score


def _with_stats(c):
    ls = Lockstep(fresh_oracle(c), c)
    elig, off, dids = eligibility(c), offsets(c), domain_ids(c)
    P = len(c["pods"])
    chosen, score = np.full(P, -1, np.int32), np.full(P, -1, np.int32)
    own_batch = opened = best_filtered = two_members = 0
    for p in range(P):
        if p % BATCH == 0:
            at_start = ls.counts.copy()
        tl, ml = c["terms"][p], c["members"][p]
        ok_now = apply_terms(tl, ls.counts)[0]
        chosen[p], score[p], free, old = ls.step(c["pods"][p], tl, ml, elig[p], off[p], int(dids[p]), stale=at_start)
        own_batch += old != chosen[p]
        opened += chosen[p] >= 0 and any(k == AFFINITY and at_start[g, chosen[p]] < q for g, k, q, _ in tl)
        best_filtered += free >= 0 and not ok_now[free]
        two_members += chosen[p] >= 0 and len(ml) == 2
    c.update(want=(chosen, score), counts_after=ls.counts[1:].astype(np.uint16),
             dcounts_after=None if ls.dom is None else ls.dom.dcounts[1:].astype(np.uint32),
             own_batch=int(own_batch), opened=int(opened), best_filtered=int(best_filtered), two_members=int(two_members),
             unplaced=int((chosen < 0).sum()), max_score=int(score.max()))
    return c


def reference(name):
    """make_input(name) with the lock-step result, computed once: want = (chosen, score), counts_after [G, n],
    dcounts_after (input X), and the statistics that keep the GPU tests from passing vacuously -- own_batch: pods that
    would have gone elsewhere had they seen the counts as they stood at the start of their 64-pod batch; opened: pods
    that landed on a node one of their AFFINITY terms had closed at the start of their batch; best_filtered: pods whose
    best node without terms was closed by a filter term when they were placed; moved: placements that differ from the
    same run without score terms; two_members: placements with two members; unplaced; max_score."""
    if ("ref", name) in _CACHE:
        return _CACHE[("ref", name)]
    c = _with_stats(dict(make_input(name)))
    ls = Lockstep(fresh_oracle(c), c)
    plain = ls.run(c["pods"], without_score_terms(c["terms"]), c["members"], eligibility(c), offsets(c), domain_ids(c))
    c["moved"] = int((plain[0] != c["want"][0]).sum())
    _CACHE[("ref", name)] = c
    return c


def affinity_only_reference():
    if "aff" not in _CACHE:
        _CACHE["aff"] = _with_stats(affinity_only_input())
    return _CACHE["aff"]


def from_groups(gids, caps):
    """§4r's group ids as term lists: terms = {ANTI(g, cap[g])}, members = {g}."""
    terms = [[(int(g), ANTI, int(caps[g - 1]), 0)] if g else [] for g in gids]
    return terms, [[int(g)] if g else [] for g in gids]


def plain_alloc(node):
    """The release record of a plain pod placed on `node` (no cpuset, NUMA, device or reservation part)."""
    a = np.zeros(1, abi.POD_ALLOCATION_DTYPE)
    a["node"] = node
    a["vf_rank"] = -1
    return a[0]


def load(ev, c):
    """The input's tables into an Evaluator; returns the keyword arguments of its schedule / submit / eval calls."""
    ev.spread_groups_load(c["counts"], np.ones(c["G"], np.uint16))  # (max_per_node is not read by term lists)
    kw = dict(spread_terms=(c["terms"], c["members"]))
    d = c["dom"]
    if d is not None:
        ev.spread_domains_load(d["maps"], d["gmap"], d["dom"], d["skew"], d["mind"], d["dcounts"])
        ev.node_sets_load(d["sets"])
        ev.node_scores_load(d["table"][None])
        kw.update(spread_domains=d["dids"], node_sets=d["sids"], node_scores=d["tids"])
    return kw


def slice_kw(kw, a, b):
    return {k: (v[0][a:b], v[1][a:b]) if k == "spread_terms" else v[a:b] for k, v in kw.items()}
