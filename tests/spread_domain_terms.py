"""Inputs and the lock-step reference of the spread domain term tests (test_spread_domain_terms_host.py pins them on
the oracle alone; test_gpu_spread_domain_terms.py runs them on the device).

A pod carries terms over the spread domain groups' counts -- SKEW (§4s's filter of the group), ANTI (node filtered when
the count of its domain >= param; a node without the topology key passes), AFFINITY (filtered at count < param, and
without the key), PREFER_FEWER / PREFER_MORE (a bonus from the clipped count; none without the key) -- and members, the
groups whose count of the node's domain, each in its own map, a placement increments.  The reference
is spread_domains' lock-step oracle with lists: per pod the oracle's eval total (+ the pod's score offset + the §4t
bonus + the domain bonus), masked with (node set), (every §4t filter term) and (every domain filter term), selectHost's
argmax, the Reserve by hand, the members' increments.
"""
import numpy as np

import spread_terms
from koordinator_amd import abi, synth
from oracle.binding import Oracle
from spread_domains import D, NONE, full_mask, open_domains
from spread_domains import make_input as domain_input
from test_node_sets_host import manual_reserve, masked_argmax

T0 = synth.T0
N_PODS = 256
WINDOW = 64  # the window the "own window" statistics refer to: what an uncut 64-pod batch would see
SKEW, ANTI, AFFINITY, FEWER, MORE = (abi.TERM_SKEW, abi.TERM_ANTI, abi.TERM_AFFINITY, abi.TERM_PREFER_FEWER,
                                     abi.TERM_PREFER_MORE)

# id -> (nodes, seed - BASE_SEED); Y: P's tables and lists on spread_terms' input X (its cluster, pods, node sets,
# score table and §4t lists)
INPUTS = {"P": (333, 9910), "Q": (600, 9920), "R": (333, 9930), "Y": (333, 9910)}
Y_CAP = 122  # what the key's range leaves a pod's score terms on input Y (make_input)
_CACHE = {}


def _maps_and_groups(name, n, rng):
    """(maps [M, n] of domain ids, groups as (map 1-based, domains mask, maxSkew, minDomains), highest seed count)."""
    zone = rng.choice(3, n, p=(0.55, 0.3, 0.15))  # spread_domains' input E: 3 zones of uneven sizes, 7 racks
    rack = rng.integers(0, 7, n)
    if name in ("P", "Y"):
        return np.stack([zone, rack]), [(1, full_mask(3), 1, 0), (1, full_mask(3), 2, 0), (2, full_mask(7), 1, 0),
                                        (2, full_mask(7), 2, 0), (1, full_mask(3), 3, 0)], 2
    m64 = rng.choice(np.setdiff1d(np.arange(64), [5, 17, 40, 63]), n)
    if name == "Q":  # 40 groups over the three maps
        shapes = [(1, full_mask(3)), (2, full_mask(7)), (3, full_mask(64))]
        return np.stack([zone, rack, m64]), [shapes[g % 3] + (1 + g % 2, 0) for g in range(40)], 2
    if name == "R":  # groups 1-3 are read (and seeded), groups 4-6 only written
        return np.stack([zone, rack, m64]), [(2, full_mask(7), 1, 0), (2, full_mask(7), 1, 0), (3, full_mask(64), 1, 0),
                                             (1, full_mask(3), 1, 0), (2, full_mask(7), 1, 0), (3, full_mask(64), 1, 0)], 3
    raise KeyError(name)


def draw_lists(rng, n_pods, G):
    """P's and Q's lists: every pod is a member of its own group, 30 % of a second one; 50 % carry SKEW on their own
    group, 25 % ANTI(other, 2..5), 20 % AFFINITY(partner, 1); 70 % carry PREFER_FEWER(own, 3..8, weight 2..10), the
    others PREFER_MORE on the partner group."""
    terms, members = [], []
    for _ in range(n_pods):
        own = int(rng.integers(1, G + 1))
        other = int(1 + (own - 1 + rng.integers(1, G)) % G)
        partner = int(1 + (own - 1 + rng.integers(1, G)) % G)
        tl, ml = [], [own]
        if rng.random() < 0.5:
            tl.append((own, SKEW, 0, 0))
        if rng.random() < 0.25:
            tl.append((other, ANTI, int(rng.integers(2, 6)), 0))
        if rng.random() < 0.2 and not any(t[0] == partner for t in tl):  # (not ANTI and AFFINITY on one group)
            tl.append((partner, AFFINITY, 1, 0))
        if rng.random() < 0.7:
            tl.append((own, FEWER, int(rng.integers(3, 9)), int(rng.integers(2, 11))))
        else:
            tl.append((partner, MORE, int(rng.integers(3, 9)), int(rng.integers(2, 11))))
        if rng.random() < 0.3:
            ml.append(other)
        terms.append(tl)
        members.append(ml)
    return terms, members


def draw_read_write_lists(rng, n_pods):
    """R's lists: a pod reads groups 1-3 -- ANTI(a, 2), AFFINITY(b, 1) and PREFER_FEWER or PREFER_MORE on c, (a, b, c)
    a permutation of them -- and is a member of one or two of groups 4-6, which nobody reads."""
    terms, members = [], []
    for _ in range(n_pods):
        a, b, c = (int(g) for g in 1 + rng.permutation(3))
        kind = FEWER if rng.random() < 0.5 else MORE
        terms.append([(a, ANTI, 2, 0), (b, AFFINITY, 1, 0), (c, kind, int(rng.integers(3, 9)), int(rng.integers(2, 11)))])
        ml = [int(4 + rng.integers(0, 3))]
        if rng.random() < 0.5:
            ml.append(int(4 + (ml[0] - 4 + rng.integers(1, 3)) % 3))
        members.append(ml)
    return terms, members


def make_input(name):
    """dict(n, cl, pods, maps [M, n] uint16, gmap / dom / skew / mind [G], dcounts [G, 64] uint32, dterms / dmembers
    (per-pod lists), and -- input Y only, else None -- x: spread_terms' input X (its dom: node sets, score table; its
    §4t counts, terms, members))."""
    if ("in", name) in _CACHE:
        return _CACHE[("in", name)]
    n, seed = INPUTS[name]
    seed += synth.BASE_SEED
    x = None
    if name == "Y":
        x = spread_terms.make_input("X")
        assert x["n"] == n
        cl, pods = x["cl"], x["pods"]
    else:
        cl = synth.make_cluster(n, seed)
        pods = synth.make_pods(N_PODS, seed + 1)
    rng = np.random.default_rng(seed + 2)
    maps, groups, top = _maps_and_groups(name, n, rng)
    maps = maps.astype(np.int64)
    maps[:, rng.random(n) < 0.05] = NONE  # nodes without the topology keys
    G = len(groups)
    dcounts = np.zeros((G, D), np.uint32)
    for g, (_, mask, _, _) in enumerate(groups):
        for d in range(D):
            if (mask >> d) & 1 and not (name == "R" and g >= 3):
                dcounts[g, d] = rng.integers(0, top + 1)
    dterms, dmembers = draw_read_write_lists(rng, N_PODS) if name == "R" else draw_lists(rng, N_PODS, G)
    if x is not None:
        # X's score table reaches 600, which leaves a pod's score terms of both kinds 1022 - 300 - 600 = 122 together
        # (a call above that is refused): a domain score term's weight is lowered to what the pod's §4t terms leave
        for p, tl in enumerate(dterms):
            left = Y_CAP - sum(t[2] * t[3] for t in x["terms"][p] if t[1] in (FEWER, MORE))
            dterms[p] = [(g, k, q, min(w, left // q) if k in (FEWER, MORE) else w) for g, k, q, w in tl]
            assert all(t[3] >= 1 for t in dterms[p] if t[1] in (FEWER, MORE))
    c = dict(n=n, cl=cl, pods=pods, maps=maps.astype(np.uint16), gmap=np.array([g[0] for g in groups], np.int32),
             dom=[g[1] for g in groups], skew=np.array([g[2] for g in groups], np.int32),
             mind=np.array([g[3] for g in groups], np.int32), dcounts=dcounts, dterms=dterms, dmembers=dmembers, x=x)
    _CACHE[("in", name)] = c
    return c


def affinity_only_input():
    """Zero seeds and AFFINITY-only pods that are members of another group: nobody can be placed."""
    c = dict(make_input("P"))
    G = len(c["gmap"])
    c["dcounts"] = np.zeros_like(c["dcounts"])
    c["dterms"] = [[(1 + p % G, AFFINITY, 1, 0)] for p in range(N_PODS)]
    c["dmembers"] = [[1 + (p + 1) % G] for p in range(N_PODS)]
    return c


def from_domain_ids(c):
    """A spread_domains input with its ids written as lists: terms = {SKEW(g)}, members = {g}."""
    c = dict(c)
    c["dterms"] = [[(int(g), SKEW, 0, 0)] if g else [] for g in c["dids"]]
    c["dmembers"] = [[int(g)] if g else [] for g in c["dids"]]
    c["x"] = None
    return c


def eligibility(c):
    return np.ones((len(c["pods"]), c["n"]), bool) if c["x"] is None else spread_terms.eligibility(c["x"])


def offsets(c):
    return np.zeros((len(c["pods"]), c["n"]), np.int64) if c["x"] is None else spread_terms.offsets(c["x"])


def node_terms(c):
    """The §4t lists per pod (terms, members): empty without input X."""
    if c["x"] is None:
        return [[]] * len(c["pods"]), [[]] * len(c["pods"])
    return c["x"]["terms"], c["x"]["members"]


def fresh_oracle(c):
    o = Oracle(synth.config(c["n"]), c["n"])
    synth.load_into(o, c["cl"])
    return o


def without_score_terms(terms):
    return [[t for t in tl if t[1] in (SKEW, ANTI, AFFINITY)] for tl in terms]


class Lockstep:
    """The reference's state: an oracle, the maps [M + 1, n] and the domain counts [G + 1, 64] (rows 0 unused) and --
    with §4t lists -- the spread groups' counts [S + 1, n]."""

    def __init__(self, o, c):
        self.o, self.n = o, c["n"]
        self.maps = np.concatenate([np.zeros((1, c["n"]), np.int64), c["maps"].astype(np.int64)])
        self.gmap = np.concatenate([[0], c["gmap"]])
        self.dom, self.skew, self.mind = [0] + list(c["dom"]), np.concatenate([[0], c["skew"]]), np.concatenate([[0], c["mind"]])
        self.dcounts = np.concatenate([np.zeros((1, D), np.int64), c["dcounts"].astype(np.int64)])
        sg = np.zeros((0, c["n"]), np.int64) if c["x"] is None else c["x"]["counts"].astype(np.int64)
        self.counts = np.concatenate([np.zeros((1, c["n"]), np.int64), sg])

    def apply(self, terms, dcounts=None):
        """(open [n] bool, bonus [n] int64) of a domain term list against the counts (`dcounts`: others than the
        current ones)."""
        dcounts = self.dcounts if dcounts is None else dcounts
        ok, bonus = np.ones(self.n, bool), np.zeros(self.n, np.int64)
        for g, kind, param, weight in terms:
            d = self.maps[self.gmap[g]]
            has = d < D
            cnt = dcounts[g][np.minimum(d, D - 1)]
            if kind == SKEW:
                ok &= has & open_domains(self.dom[g], self.skew[g], self.mind[g], dcounts[g])[np.minimum(d, D - 1)]
            elif kind == ANTI:
                ok &= ~has | (cnt < param)
            elif kind == AFFINITY:
                ok &= has & (cnt >= param)
            elif kind == FEWER:
                bonus += np.where(has, weight * (param - np.minimum(cnt, param)), 0)
            elif kind == MORE:
                bonus += np.where(has, weight * np.minimum(cnt, param), 0)
            else:
                raise ValueError(kind)
        return ok, bonus

    def pick(self, total, off, terms, base, dcounts=None):
        ok, bonus = self.apply(terms, dcounts)
        return masked_argmax(np.where(total >= 0, total + off + bonus, -1), base & ok)

    def step(self, pod, terms, members, elig, off, sterms=(), smembers=(), stale=None):
        """Place one pod; returns (node, score, the best node by set, offset and §4t lists alone or -1, the node the pod
        would have taken had the domain counts been `stale` -- None: not asked for)."""
        total = self.o.eval(pod.reshape(1), T0)["total"][0].astype(np.int64)
        sok, sbonus = spread_terms.apply_terms(sterms, self.counts)
        base, off = elig & sok, off + sbonus
        free, _ = masked_argmax(np.where(total >= 0, total + off, -1), base)
        old = None if stale is None else self.pick(total, off, terms, base, stale)[0]
        node, score = self.pick(total, off, terms, base)
        if node >= 0:
            manual_reserve(self.o, node, pod)
            for m in smembers:
                self.counts[m, node] = min(self.counts[m, node] + 1, spread_terms.SAT)
            for m in members:
                d = self.maps[self.gmap[m], node]
                if d < D:
                    self.dcounts[m, d] += 1
        return node, score, free, old

    def run(self, pods, terms, members, elig, off, sterms=None, smembers=None):
        chosen, score = np.full(len(pods), -1, np.int32), np.full(len(pods), -1, np.int32)
        for p in range(len(pods)):
            chosen[p], score[p] = self.step(pods[p], terms[p], members[p], elig[p], off[p],
                                            () if sterms is None else sterms[p], () if smembers is None else smembers[p])[:2]
        return chosen, score


def _with_stats(c):
    ls = Lockstep(fresh_oracle(c), c)
    elig, off = eligibility(c), offsets(c)
    sterms, smembers = node_terms(c)
    P = len(c["pods"])
    chosen, score = np.full(P, -1, np.int32), np.full(P, -1, np.int32)
    own_window = best_filtered = newly = same_node = cell_hits = increments = 0
    for p in range(P):
        if p % WINDOW == 0:
            at_start = ls.dcounts.copy()
            taken, cells = set(), set()
        tl, ml = c["dterms"][p], c["dmembers"][p]
        ok_now, ok_then = ls.apply(tl)[0], ls.apply(tl, at_start)[0]
        chosen[p], score[p], free, old = ls.step(c["pods"][p], tl, ml, elig[p], off[p], sterms[p], smembers[p], stale=at_start)
        own_window += old != chosen[p]
        best_filtered += free >= 0 and not ok_now[free]
        node = int(chosen[p])
        if node < 0:
            continue
        newly += not ok_then[node]
        same_node += node in taken
        taken.add(node)
        for m in ml:
            d = int(ls.maps[ls.gmap[m], node])
            if d < D:
                increments += 1
                cell_hits += (m, d) in cells
                cells.add((m, d))
    sizes = plan(c["dterms"], c["dmembers"], WINDOW)
    c.update(want=(chosen, score), dcounts_after=ls.dcounts[1:].astype(np.uint32),
             counts_after=ls.counts[1:].astype(np.uint16), own_window=int(own_window), best_filtered=int(best_filtered),
             newly=int(newly), same_node=int(same_node), cell_hits=int(cell_hits), increments=int(increments),
             unplaced=int((chosen < 0).sum()), max_score=int(score.max()), batches=len(sizes), longest=max(sizes))
    return c


def reference(name):
    """make_input(name) with the lock-step result, computed once: want = (chosen, score), dcounts_after [G, 64],
    counts_after (§4t), and the statistics that keep the GPU tests from passing vacuously -- own_window: pods that would
    have gone elsewhere had they seen the domain counts as they stood at the start of their 64-pod window (what an uncut
    batch computes); best_filtered: pods whose best node without domain terms was closed by one when they were placed;
    newly: pods that landed on a node closed to them at the start of their window; same_node: pods that landed on a node
    taken earlier in their window; increments / cell_hits: member increments, and those that hit a (group, domain) cell
    already hit in their window; score_moved: placements that differ from the same run without domain score terms;
    unplaced; max_score; batches / longest: the plan at batch 64."""
    if ("ref", name) in _CACHE:
        return _CACHE[("ref", name)]
    c = _with_stats(dict(make_input(name)))
    ls = Lockstep(fresh_oracle(c), c)
    plain = ls.run(c["pods"], without_score_terms(c["dterms"]), c["dmembers"], eligibility(c), offsets(c), *node_terms(c))
    c["score_moved"] = int((plain[0] != c["want"][0]).sum())
    _CACHE[("ref", name)] = c
    return c


def affinity_only_reference():
    if "aff" not in _CACHE:
        _CACHE["aff"] = _with_stats(affinity_only_input())
    return _CACHE["aff"]


def id_equivalent_reference(name):
    """spread_domains' input `name` with its ids as lists, run through this module's Lockstep: (input, (chosen, score),
    dcounts_after)."""
    if ("ids", name) not in _CACHE:
        c = from_domain_ids(domain_input(name))
        ls = Lockstep(fresh_oracle(c), c)
        got = ls.run(c["pods"], c["dterms"], c["dmembers"], eligibility(c), offsets(c))
        _CACHE[("ids", name)] = (c, got, ls.dcounts[1:].astype(np.uint32))
    return _CACHE[("ids", name)]


def plan(terms, members, batch):
    """ke_plan.h's segmentation of a plain queue with domain lists restated: the pod count of every batch -- up to
    `batch` pods, ended before a pod one of whose term groups is a member group of an earlier pod of the batch."""
    out, written, cur = [], set(), 0
    for tl, ml in zip(terms, members):
        if cur == batch or any(t[0] in written for t in tl):
            out.append(cur)
            written, cur = set(), 0
        cur += 1
        written.update(int(m) for m in ml)
    return out + [cur] if cur else out


def load(ev, c):
    """The input's tables into an Evaluator; returns the keyword arguments of its schedule / submit / eval calls."""
    ev.spread_domains_load(c["maps"], c["gmap"], c["dom"], c["skew"], c["mind"], c["dcounts"])
    kw = dict(spread_domain_terms=(c["dterms"], c["dmembers"]))
    x = c["x"]
    if x is not None:
        ev.spread_groups_load(x["counts"], np.ones(x["G"], np.uint16))
        ev.node_sets_load(x["dom"]["sets"])
        ev.node_scores_load(x["dom"]["table"][None])
        kw.update(spread_terms=(x["terms"], x["members"]), node_sets=x["dom"]["sids"], node_scores=x["dom"]["tids"])
    return kw


def slice_kw(kw, a, b):
    return {k: (v[0][a:b], v[1][a:b]) if k in ("spread_terms", "spread_domain_terms") else v[a:b] for k, v in kw.items()}
