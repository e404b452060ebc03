"""Spread domain terms: what a queue with domain term lists costs on the config-3 workload.

The same cluster and queue (BASELINE config 3: 50k nodes x 100k pods) scheduled through the submit-ahead loop of
bench.py (ke_schedule_submit of step s+1 before ke_schedule_wait of step s), with a table of 8 spread domain groups
(maxSkew 1, zero seeds) over zone = node mod 3 loaded every time, and these workloads: every list empty (the kernels and
the pipelined schedule of a call without lists); every pod with SKEW(g) + member g on a random group g of 1..8 -- §4s's
all-grouped workload as lists, the same plan -- and, beside it, the same ids through ke_pod_spread_domains; every pod
with PREFER_FEWER(g) + member g (the ScheduleAnyway default, the same cuts); and a read-only / write-only workload --
every pod reads two of groups 1..4 (ANTI with a param no count reaches, PREFER_FEWER) and is a member of one of groups
5..8, so no batch is cut.  The kinds alternate, `--repeats` runs each.  A bounded prefix of the PREFER_FEWER workload is
checked against a lock-step oracle.  The lists are packed into the entry point's arrays ahead of the timed loop.  Prints
one JSON line.
Usage: python tools/spread_domain_terms_bench.py [--nodes 50000 --pods 100000 --steps 20 --warmup 5 --groups 8 --zones 3 --repeats 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from koordinator_amd import Evaluator, abi, synth  # noqa: E402


class Lists:
    """Per-pod lists with the same number of terms (k) and members (m) on every pod, as the entry point's arrays."""

    def __init__(self, terms, members):
        self.terms = np.ascontiguousarray(terms, np.int32)  # [P, k, 4]
        self.members = np.ascontiguousarray(members, np.int32)  # [P, m]
        self.k, self.m = self.terms.shape[1], self.members.shape[1]

    def stage(self, ev, a, b):
        n = b - a
        t_off = np.arange(n + 1, dtype=np.int32) * self.k
        m_off = np.arange(n + 1, dtype=np.int32) * self.m
        t = np.ascontiguousarray(self.terms[a:b])
        m = np.ascontiguousarray(self.members[a:b])
        ev._check(ev.lib.ke_pod_spread_domain_terms(ev.h, n, abi.ptr(t_off), abi.ptr(t) if t.size else None,
                                                    abi.ptr(m_off), abi.ptr(m) if m.size else None))

    def python(self, a, b):
        return [[tuple(int(v) for v in t) for t in tl] for tl in self.terms[a:b]], [list(map(int, m)) for m in self.members[a:b]]


class Ids:
    """§4s's form of the SKEW(g) + {g} workload: spread domain group ids."""

    def __init__(self, ids):
        self.ids = np.ascontiguousarray(ids, np.int32)

    def stage(self, ev, a, b):
        ev.pod_spread_domains(self.ids[a:b])


def run(cfg, cl, table, pods, lists, steps, warmup):
    def fresh():
        ev = Evaluator(cfg)
        synth.load_into(ev, cl)
        ev.spread_domains_load(*table)
        return ev

    sl = len(pods) // steps
    if warmup > 0:  # a throwaway context, other pods
        ew = fresh()
        wp = synth.make_pods(warmup * sl, synth.BASE_SEED + 203)
        for w in range(warmup):
            lists.stage(ew, w * sl, (w + 1) * sl)
            ew.schedule(wp[w * sl:(w + 1) * sl], synth.T0)
        ew.close()
    ev = fresh()
    ev.eval(pods[:0], synth.T0)  # every node row resident in HBM
    ev.set_profiling(8)  # (as bench.py: HIP-event samples of every 8th batch's kernels)

    def submit(s):
        lists.stage(ev, s * sl, (s + 1) * sl)
        return ev.submit(pods[s * sl:(s + 1) * sl], synth.T0)

    placed, npipe, nbatch, kss = 0, 0, 0, []
    t0 = time.perf_counter()
    nxt = submit(0)
    for s in range(steps):
        cur = nxt
        nxt = submit(s + 1) if s + 1 < steps else None
        chosen, _ = ev.wait(cur)
        placed += int((chosen >= 0).sum())
        kss.append(ev.kernel_stats())
        npipe += kss[-1]["pipelined_batches"]
        nbatch += len(ev.stats()[1])
    dt = time.perf_counter() - t0
    mismatched = ev.debug_spread_domains_check()
    ev.close()
    n = steps * sl
    mean = lambda key: float(np.mean([k[key] for k in kss]))  # noqa: E731
    return {"value": n * cl.n_nodes / dt, "ms_per_pod": dt / n * 1e3, "placed": placed, "batches": nbatch,
            "pipelined_batches": npipe, "count_mismatches": mismatched,
            # per batch: the sampled eval and select kernels, the Reserve chain, its wait for the lists
            "kernel_ms_per_batch": {k: mean(k) for k in ("eval_ms", "select_ms", "resolve_ms", "handoff_ms")}}


def oracle_prefix(cfg, cl, table, pods, lists, n):
    from oracle.binding import Oracle  # checker only

    zone = table[0]
    ev, o = Evaluator(cfg), Oracle(cfg, cl.n_nodes)
    synth.load_into(ev, cl)
    synth.load_into(o, cl)
    ev.spread_domains_load(*table)
    terms, members = lists.python(0, n)
    c1, s1 = ev.schedule(pods[:n], synth.T0, spread_domain_terms=(terms, members))
    counts = np.zeros((len(table[1]) + 1, int(zone.max()) + 1), np.int64)
    for p in range(n):
        t = o.eval(pods[p:p + 1], synth.T0, n_threads=16)["total"][0].astype(np.int64)
        for g, kind, param, weight in terms[p]:
            assert kind == abi.TERM_PREFER_FEWER
            t = np.where(t >= 0, t + weight * (param - np.minimum(counts[g], param))[zone[0]], -1)
        node = int(np.argmax(t))
        want = (node, int(t[node])) if t[node] >= 0 else (-1, -1)
        if (int(c1[p]), int(s1[p])) != want:
            return False
        if t[node] >= 0:
            o.assign_bulk([node], pods[p:p + 1], [synth.T0])
            req = o.node_info_requested(node)[0]
            o.set_requested(node, int(req[0]) + int(pods["requests"][p, abi.RES_CPU]),
                            int(req[1]) + int(pods["requests"][p, abi.RES_MEMORY]))
            for m in members[p]:
                counts[m, zone[0, node]] += 1
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=synth.CONFIGS[3]["nodes"])
    ap.add_argument("--pods", type=int, default=synth.CONFIGS[3]["pods"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--zones", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=2, help="runs of each kind, alternating (the best of each is reported)")
    ap.add_argument("--kinds", default="lists_all_empty,skew_member,skew_ids,fewer_member,read_write")
    ap.add_argument("--check-pods", type=int, default=128, help="lock-step oracle prefix of the PREFER_FEWER run (0 = off)")
    a = ap.parse_args()
    assert a.groups >= 2 and a.groups % 2 == 0
    cl = synth.make_cluster(a.nodes, synth.BASE_SEED + 3)
    pods = synth.make_pods(a.pods, synth.BASE_SEED + 103)
    rng = np.random.default_rng(synth.BASE_SEED + 1504)
    # (maps, each group's map, its domains -- every zone --, its maxSkew): §4s's bench table
    table = (np.arange(a.nodes)[None] % a.zones, np.ones(a.groups, np.int32), [(1 << a.zones) - 1] * a.groups,
             np.ones(a.groups, np.int32))
    g = rng.integers(1, a.groups + 1, a.pods).astype(np.int32)  # (§4s's bench draws the same ids)
    zero = np.zeros(a.pods, np.int32)
    half = a.groups // 2
    ra, rb = rng.integers(1, half + 1, a.pods).astype(np.int32), rng.integers(1, half + 1, a.pods).astype(np.int32)
    w = (half + rng.integers(1, half + 1, a.pods)).astype(np.int32)
    skew = np.stack([g, zero + abi.TERM_SKEW, zero, zero], 1)
    fewer = np.stack([g, zero + abi.TERM_PREFER_FEWER, zero + 8, zero + 10], 1)
    anti = np.stack([ra, zero + abi.TERM_ANTI, zero + 65535, zero], 1)
    rfewer = np.stack([rb, zero + abi.TERM_PREFER_FEWER, zero + 8, zero + 10], 1)
    kinds = {"lists_all_empty": Lists(np.zeros((a.pods, 0, 4), np.int32), np.zeros((a.pods, 0), np.int32)),
             "skew_member": Lists(skew[:, None, :], g[:, None]),
             "skew_ids": Ids(g),
             "fewer_member": Lists(fewer[:, None, :], g[:, None]),
             "read_write": Lists(np.stack([anti, rfewer], 1), w[:, None])}
    kinds = {k: v for k, v in kinds.items() if k in a.kinds.split(",")}
    cfg = synth.config(a.nodes)
    runs = [{k: run(cfg, cl, table, pods, ls, a.steps, a.warmup) for k, ls in kinds.items()}
            for _ in range(max(1, a.repeats))]
    best = {k: max((r[k] for r in runs), key=lambda r: r["value"]) for k in kinds}
    out = {"workload": f"{a.nodes} nodes x {a.pods} pods (config-3 shape), {a.groups} spread domain groups of maxSkew 1 "
                       f"over {a.zones} zones",
           "unit": "pod-node evals/s", **best, "all_values": {k: [r[k]["value"] for r in runs] for k in kinds}}
    if a.check_pods and "fewer_member" in kinds:
        out["oracle_prefix_equal"] = oracle_prefix(cfg, cl, table, pods, kinds["fewer_member"], a.check_pods)
        out["oracle_prefix_pods"] = a.check_pods
    print(json.dumps(out))


if __name__ == "__main__":
    main()
