"""Every legal combination of a call's per-pod attachments on one small slice: input X of spread_terms.py (333 nodes:
more than one set-table word and more than one wave of counts; spread_domains' input E with node sets, a score table
and domain ids) and its first 48 pods, which pod_batch = 16 splits into three batches or more.  A combination is
(sets, scores, domains, gt) with gt 0 = neither, 1 = spread group ids, 2 = spread term lists; a kind left out is not
passed.  Group ids are each pod's first member with cap 1 over the input's seeded counts, and their reference is
spread_terms.from_groups through its Lockstep, as for the lists.  test_attachments_host.py pins the references on the
oracle alone, test_gpu_attachments.py runs them on the device."""
import numpy as np

from koordinator_amd import synth
from spread_terms import (Lockstep, apply_terms, domain_ids, eligibility, fresh_oracle, from_groups, make_input,
                          offsets)
from test_node_sets_host import masked_argmax, sub_oracle

T0 = synth.T0
P = 48
BATCH = 16
N_EVAL = 4
COMBOS = [(s, c, d, gt) for s in (0, 1) for c in (0, 1) for d in (0, 1) for gt in (0, 1, 2)]
_CACHE = {}


def combo_id(combo):
    s, c, d, gt = combo
    return "-".join(n for n, on in (("sets", s), ("scores", c), ("domains", d), ("groups", gt == 1), ("terms", gt == 2))
                    if on) or "none"


def without(combo, kind):
    """The combination with one present kind dropped."""
    k = list(combo)
    assert k[kind]
    k[kind] = 0
    return tuple(k)


def inputs(combo):
    """dict(c: input X, pods, kw: the keywords of Evaluator.eval / schedule, and the reference's view of them -- terms,
    members (per-pod lists), elig [P, n] bool, off [P, n] int64, dids [P])."""
    sets, scores, domains, gt = combo
    c = make_input("X")
    d = c["dom"]
    n = c["n"]
    kw = {}
    terms, members = [[] for _ in range(P)], [[] for _ in range(P)]
    if gt == 1:
        gids = np.array([c["members"][p][0] for p in range(P)], np.int32)
        kw["spread_groups"] = gids
        terms, members = from_groups(gids, np.ones(c["G"], np.uint16))
    elif gt == 2:
        terms, members = c["terms"][:P], c["members"][:P]
        kw["spread_terms"] = (terms, members)
    elig, off, dids = np.ones((P, n), bool), np.zeros((P, n), np.int64), np.zeros(P, np.int32)
    if sets:
        kw["node_sets"] = d["sids"][:P]
        elig = eligibility(c)[:P]
    if scores:
        kw["node_scores"] = d["tids"][:P]
        off = offsets(c)[:P]
    if domains:
        kw["spread_domains"] = d["dids"][:P]
        dids = domain_ids(c)[:P]
    return dict(c=c, pods=c["pods"][:P], kw=kw, terms=terms, members=members, elig=elig, off=off, dids=dids)


def reference(combo):
    """inputs(combo) with the lock-step result, computed once: want = (chosen, score), counts_after [G, n] uint16 and
    dcounts_after [groups, 64] uint32 (the seeds where the combination has no kind that moves them)."""
    if combo not in _CACHE:
        r = inputs(combo)
        ls = Lockstep(fresh_oracle(r["c"]), r["c"])
        r["want"] = ls.run(r["pods"], r["terms"], r["members"], r["elig"], r["off"], r["dids"])
        r["counts_after"] = ls.counts[1:].astype(np.uint16)
        r["dcounts_after"] = ls.dom.dcounts[1:].astype(np.uint32)
        _CACHE[combo] = r
    return _CACHE[combo]


def eval_reference(combo):
    """ke_eval of the first N_EVAL pods against the loaded tables: (best [N_EVAL], total [N_EVAL, n]).  A pod's open
    nodes are those of its set, of an open domain and past every filter term; their totals are the oracle's over the
    sub-cluster of the open nodes, plus the pod's table entry and the bonus; every other pair is -1."""
    r = inputs(combo)
    c = r["c"]
    n = c["n"]
    ls = Lockstep(None, c)
    best, total = np.full(N_EVAL, -1, np.int32), np.full((N_EVAL, n), -1, np.int64)
    for p in range(N_EVAL):
        ok, bonus = apply_terms(r["terms"][p], ls.counts)
        idx = np.nonzero(ok & r["elig"][p] & ls.domain_ok(int(r["dids"][p])))[0]
        if len(idx) == 0:
            continue
        t = sub_oracle(synth.config, c["cl"], idx).eval(r["pods"][p:p + 1], T0)["total"][0].astype(np.int64)
        total[p, idx] = np.where(t >= 0, t + r["off"][p][idx] + bonus[idx], -1)
        best[p] = masked_argmax(total[p], np.ones(n, bool))[0]
    return best, total
