"""Spread terms: what a queue with term lists costs on the config-3 workload.

The same cluster and queue (BASELINE config 3: 50k nodes x 100k pods) scheduled through the submit-ahead loop of
bench.py (ke_schedule_submit of step s+1 before ke_schedule_wait of step s), with a table of 8 spread groups (zero
initial counts) loaded every time, and three workloads: every list empty (the kernels and the pipelined schedule of a
call without lists), every pod with ANTI(g, cap) + member g on a random group g of 1..8 (§4r's all-grouped workload as
term lists: every batch serial, on the one-wave sequential replay), and the same plus a PREFER_FEWER term on g.  The
kinds alternate, `--repeats` runs each.  A bounded prefix of the last workload is checked against a lock-step oracle.
The lists are packed into the entry point's arrays ahead of the timed loop.  Prints one JSON line.
Usage: python tools/spread_terms_bench.py [--nodes 50000 --pods 100000 --steps 20 --warmup 5 --groups 8 --cap 2 --repeats 2]
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
        ev._check(ev.lib.ke_pod_spread_terms(ev.h, n, abi.ptr(t_off), abi.ptr(t) if t.size else None, abi.ptr(m_off),
                                             abi.ptr(m) if m.size else None))

    def python(self, a, b):
        return [[tuple(int(v) for v in t) for t in tl] for tl in self.terms[a:b]], [list(map(int, m)) for m in self.members[a:b]]


def run(cfg, cl, groups, pods, lists, steps, warmup):
    def fresh():
        ev = Evaluator(cfg)
        synth.load_into(ev, cl)
        ev.spread_groups_load(None, np.ones(groups, np.uint16))
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

    placed, npipe, kss = 0, 0, []
    t0 = time.perf_counter()
    nxt = submit(0)
    for s in range(steps):
        cur = nxt
        nxt = submit(s + 1) if s + 1 < steps else None
        chosen, _ = ev.wait(cur)
        placed += int((chosen >= 0).sum())
        kss.append(ev.kernel_stats())
        npipe += kss[-1]["pipelined_batches"]
    dt = time.perf_counter() - t0
    mismatched = ev.debug_spread_groups_check()
    ev.close()
    n = steps * sl
    mean = lambda key: float(np.mean([k[key] for k in kss]))  # noqa: E731
    return {"value": n * cl.n_nodes / dt, "ms_per_pod": dt / n * 1e3, "placed": placed, "pipelined_batches": npipe,
            "count_mismatches": mismatched,
            # per batch: the sampled eval and select kernels, the Reserve chain, its wait for the lists
            "kernel_ms_per_batch": {k: mean(k) for k in ("eval_ms", "select_ms", "resolve_ms", "handoff_ms")}}


def oracle_prefix(cfg, cl, groups, pods, lists, n):
    from oracle.binding import Oracle  # checker only

    ev, o = Evaluator(cfg), Oracle(cfg, cl.n_nodes)
    synth.load_into(ev, cl)
    synth.load_into(o, cl)
    ev.spread_groups_load(None, np.ones(groups, np.uint16))
    terms, members = lists.python(0, n)
    c1, s1 = ev.schedule(pods[:n], synth.T0, spread_terms=(terms, members))
    counts = np.zeros((groups + 1, cl.n_nodes), np.int64)
    for p in range(n):
        t = o.eval(pods[p:p + 1], synth.T0, n_threads=16)["total"][0].astype(np.int64)
        ok = np.ones(cl.n_nodes, bool)
        for g, kind, param, weight in terms[p]:
            if kind == abi.TERM_ANTI:
                ok &= counts[g] < param
            elif kind == abi.TERM_PREFER_FEWER:
                t = np.where(t >= 0, t + weight * (param - np.minimum(counts[g], param)), -1)
        t = np.where(ok, t, -1)
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
                counts[m, node] += 1
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=synth.CONFIGS[3]["nodes"])
    ap.add_argument("--pods", type=int, default=synth.CONFIGS[3]["pods"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--cap", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=2, help="runs of each kind, alternating (the best of each is reported)")
    ap.add_argument("--check-pods", type=int, default=128, help="lock-step oracle prefix of the last workload (0 = off)")
    a = ap.parse_args()
    cl = synth.make_cluster(a.nodes, synth.BASE_SEED + 3)
    pods = synth.make_pods(a.pods, synth.BASE_SEED + 103)
    rng = np.random.default_rng(synth.BASE_SEED + 1503)
    g = rng.integers(1, a.groups + 1, a.pods).astype(np.int32)  # (§4r's bench draws the same ids)
    zero = np.zeros(a.pods, np.int32)
    anti = np.stack([g, zero + abi.TERM_ANTI, zero + a.cap, zero], 1)
    fewer = np.stack([g, zero + abi.TERM_PREFER_FEWER, zero + a.cap, zero + 10], 1)
    kinds = {"lists_all_empty": Lists(np.zeros((a.pods, 0, 4), np.int32), np.zeros((a.pods, 0), np.int32)),
             "anti_member": Lists(anti[:, None, :], g[:, None]),
             "anti_member_fewer": Lists(np.stack([anti, fewer], 1), g[:, None])}
    cfg = synth.config(a.nodes)
    runs = [{k: run(cfg, cl, a.groups, pods, ls, a.steps, a.warmup) for k, ls in kinds.items()}
            for _ in range(max(1, a.repeats))]
    best = {k: max((r[k] for r in runs), key=lambda r: r["value"]) for k in kinds}
    out = {"workload": f"{a.nodes} nodes x {a.pods} pods (config-3 shape), {a.groups} spread groups, ANTI param {a.cap}",
           "unit": "pod-node evals/s", **best,
           "anti_member_cost": best["lists_all_empty"]["value"] / best["anti_member"]["value"],
           "anti_member_fewer_cost": best["lists_all_empty"]["value"] / best["anti_member_fewer"]["value"],
           "all_values": {k: [r[k]["value"] for r in runs] for k in kinds}}
    if a.check_pods:
        out["oracle_prefix_equal"] = oracle_prefix(cfg, cl, a.groups, pods, kinds["anti_member_fewer"], a.check_pods)
        out["oracle_prefix_pods"] = a.check_pods
    print(json.dumps(out))


if __name__ == "__main__":
    main()
