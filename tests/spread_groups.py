"""Inputs and the lock-step reference of the spread group tests (test_spread_groups_host.py pins them on the oracle
alone; test_gpu_spread_groups.py runs them on the device).

A spread group g has a cap and a pod count per node; a node whose count has reached the cap is filtered for the
group's pods, and every placement of such a pod increments its node's count.  The reference is the
node sets' lock-step oracle with that one more piece of state: per pod the oracle's eval total (+ the pod's score
offset), masked with (node set) and (count[g] < cap[g]), selectHost's argmax, the Reserve by hand, count[g][node] += 1.
"""
import numpy as np

from koordinator_amd import abi, synth
from landscapes import HOT_NODES, HOT_OFFSETS
from oracle.binding import Oracle
from test_node_sets_host import manual_reserve, masked_argmax

T0 = synth.T0
N_PODS = 256
BATCH = 64  # the batch the "depends on its own batch" statistics refer to

# id -> (nodes, seed - BASE_SEED, caps of groups 1..G)
INPUTS = {"A": (333, 9600, (1, 1, 2, 3)), "B": (333, 9610, (1, 2)), "C": (130, 9620, (1, 1)), "D": (600, 9630, (1, 2, 2))}
_CACHE = {}


def make_input(name):
    """dict(n, cl, pods, gids [P], caps [G], counts [G, n] uint16, and -- input D only, else None -- sets [2, n] bool,
    sids [P], table [n], tids [P])."""
    if ("in", name) in _CACHE:
        return _CACHE[("in", name)]
    n, seed, caps = INPUTS[name]
    seed += synth.BASE_SEED
    G = len(caps)
    cl = synth.make_cluster(n, seed)
    pods = synth.make_pods(N_PODS, seed + 1)
    rng = np.random.default_rng(seed + 2)
    # (one draw of the grouped fraction for every input -- 0.75 for A, every pod elsewhere -- then the ids)
    gids = np.where(rng.random(N_PODS) < (0.75 if name == "A" else 1.0), rng.integers(1, G + 1, N_PODS), 0)
    counts = rng.random((G + 1, n)) < 0.15
    counts[0] = False
    counts = counts[1:].astype(np.uint16)
    sets = sids = table = tids = None
    if name == "D":  # zero initial counts; node sets and score offsets besides
        counts[:] = 0
        sids = rng.integers(0, 3, N_PODS)
        sets = rng.random((2, n)) < 0.5
        sets[:, list(HOT_NODES)] = True
        table = np.zeros(n, np.int64)
        table[list(HOT_NODES)] = HOT_OFFSETS
        tids = np.ones(N_PODS, np.int32)
    c = dict(n=n, cl=cl, pods=pods, gids=gids.astype(np.int32), caps=np.asarray(caps, np.uint16), counts=counts,
             sets=sets, sids=None if sids is None else sids.astype(np.int32), table=table, tids=tids)
    _CACHE[("in", name)] = c
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


def fresh_oracle(c):
    o = Oracle(synth.config(c["n"]), c["n"])
    synth.load_into(o, c["cl"])
    return o


class Lockstep:
    """The reference's state: an oracle and the counts [G + 1, n] (row 0 stays zero; caps[0] is never reached)."""

    def __init__(self, o, counts, caps):
        self.o = o
        self.counts = np.concatenate([np.zeros((1, counts.shape[1]), np.int64), counts.astype(np.int64)])
        self.caps = np.concatenate([[1 << 30], np.asarray(caps, np.int64)])

    def step(self, pod, gid, elig, off, stale=None):
        """Place one pod; returns (node, score, the best node by the node set alone or -1, the node the pod would
        have taken had the counts been `stale` -- None: not asked for)."""
        total = self.o.eval(pod.reshape(1), T0)["total"][0].astype(np.int64)
        total = np.where(total >= 0, total + off, -1)
        free, _ = masked_argmax(total, elig)
        old = None if stale is None else masked_argmax(total, elig & (stale[gid] < self.caps[gid]))[0]
        node, score = masked_argmax(total, elig & (self.counts[gid] < self.caps[gid]))
        if node >= 0:
            manual_reserve(self.o, node, pod)
            self.counts[gid, node] += 1
        return node, score, free, old

    def run(self, pods, gids, elig, off):
        chosen, score = np.full(len(pods), -1, np.int32), np.full(len(pods), -1, np.int32)
        for p in range(len(pods)):
            chosen[p], score[p] = self.step(pods[p], int(gids[p]), elig[p], off[p])[:2]
        return chosen, score


def reference(name):
    """make_input(name) with the lock-step result, computed once: want = (chosen, score), counts_after [G, n], and the
    statistics that keep the GPU tests from passing vacuously -- best_capped: pods whose best node by their node set
    alone was capped when they were placed; own_batch: pods that depend on their own 64-pod batch's increments, i.e.
    that would have gone elsewhere had they seen the counts as they stood at the start of their batch (a site that
    ignores the cap or reads a stale count moves these); unplaced."""
    if ("ref", name) in _CACHE:
        return _CACHE[("ref", name)]
    c = dict(make_input(name))
    ls = Lockstep(fresh_oracle(c), c["counts"], c["caps"])
    elig, off = eligibility(c), offsets(c)
    P = len(c["pods"])
    chosen, score = np.full(P, -1, np.int32), np.full(P, -1, np.int32)
    best_capped = own_batch = 0
    for p in range(P):
        if p % BATCH == 0:
            at_batch_start = ls.counts.copy()
        g = int(c["gids"][p])
        capped_now = ls.counts[g] >= ls.caps[g]
        chosen[p], score[p], free, old = ls.step(c["pods"][p], g, elig[p], off[p], stale=at_batch_start)
        best_capped += free >= 0 and bool(capped_now[free])
        own_batch += old != chosen[p]
    c.update(want=(chosen, score), counts_after=ls.counts[1:].astype(np.uint16), best_capped=best_capped,
             own_batch=int(own_batch), unplaced=int((chosen < 0).sum()))
    _CACHE[("ref", name)] = c
    return c


def reference_without_groups(name):
    """The same run with every group id 0 (node sets and offsets kept): (chosen, score)."""
    if ("nogroups", name) not in _CACHE:
        c = make_input(name)
        ls = Lockstep(fresh_oracle(c), c["counts"], c["caps"])
        _CACHE[("nogroups", name)] = ls.run(c["pods"], np.zeros(len(c["pods"]), np.int32), eligibility(c), offsets(c))
    return _CACHE[("nogroups", name)]


def plain_alloc(node):
    """The release record of a plain pod placed on `node` (no cpuset, NUMA, device or reservation part)."""
    a = np.zeros(1, abi.POD_ALLOCATION_DTYPE)
    a["node"] = node
    a["vf_rank"] = -1
    return a[0]


def load(ev, c):
    """The input's tables into an Evaluator; returns the keyword arguments of its schedule / submit / eval calls."""
    ev.spread_groups_load(c["counts"], c["caps"])
    kw = dict(spread_groups=c["gids"])
    if c["sets"] is not None:
        ev.node_sets_load(c["sets"])
        ev.node_scores_load(c["table"][None])
        kw.update(node_sets=c["sids"], node_scores=c["tids"])
    return kw


def slice_kw(kw, a, b):
    return {k: v[a:b] for k, v in kw.items()}
