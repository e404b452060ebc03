"""Spread domains: what a queue with spread domain ids costs on the config-3 workload.

The same cluster and queue (BASELINE config 3: 50k nodes x 100k pods) scheduled through the submit-ahead loop of
bench.py (ke_schedule_submit of step s+1 before ke_schedule_wait of step s), with 8 spread domain groups of maxSkew 1
over a 3-zone map (zone = node mod 3, zero seeds) loaded every time: with every pod's id 0 (the kernels and the
pipelined schedule of a call without ids), with every pod in a random group 1..8 (a batch ends at the first repeated
group), with 10 % of the pods grouped, and with every pod in group 1 (the worst case: every batch is a singleton).  A
bounded prefix of the all-grouped run is checked against a lock-step oracle (argmax of its eval over the nodes of the
open zones, the Reserve, the count).  Prints one JSON line.
Usage: python tools/spread_domains_bench.py [--nodes 50000 --pods 100000 --steps 20 --warmup 5 --groups 8 --zones 3]
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


def run(cfg, cl, table, pods, ids, steps, warmup):
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
            ew.schedule(wp[w * sl:(w + 1) * sl], synth.T0, spread_domains=ids[w * sl:(w + 1) * sl])
        ew.close()
    ev = fresh()
    ev.eval(pods[:0], synth.T0)  # every node row resident in HBM
    ev.set_profiling(8)  # (as bench.py: HIP-event samples of every 8th batch's kernels)
    part = lambda s: (pods[s * sl:(s + 1) * sl], synth.T0, ids[s * sl:(s + 1) * sl])  # noqa: E731
    placed, npipe, nbatch, kss = 0, 0, 0, []
    t0 = time.perf_counter()
    nxt = ev.submit(part(0)[0], part(0)[1], spread_domains=part(0)[2])
    for s in range(steps):
        cur = nxt
        nxt = ev.submit(part(s + 1)[0], part(s + 1)[1], spread_domains=part(s + 1)[2]) if s + 1 < steps else None
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


def oracle_prefix(cfg, cl, table, pods, ids, n):
    from oracle.binding import Oracle  # checker only

    zone, _, dom, skew = table
    ev, o = Evaluator(cfg), Oracle(cfg, cl.n_nodes)
    synth.load_into(ev, cl)
    synth.load_into(o, cl)
    ev.spread_domains_load(*table)
    c1, s1 = ev.schedule(pods[:n], synth.T0, spread_domains=ids[:n])
    Z = int(zone.max()) + 1
    counts = np.zeros((len(dom) + 1, Z), np.int64)
    for p in range(n):
        g = int(ids[p])
        t = o.eval(pods[p:p + 1], synth.T0, n_threads=16)["total"][0].astype(np.int64)
        if g:
            t = np.where((counts[g] + 1 - counts[g].min() <= skew[g - 1])[zone[0]], t, -1)
        node = int(np.argmax(t))
        want = (node, int(t[node])) if t[node] >= 0 else (-1, -1)
        if (int(c1[p]), int(s1[p])) != want:
            return False
        if t[node] >= 0:
            o.assign_bulk([node], pods[p:p + 1], [synth.T0])
            req = o.node_info_requested(node)[0]
            o.set_requested(node, int(req[0]) + int(pods["requests"][p, abi.RES_CPU]),
                            int(req[1]) + int(pods["requests"][p, abi.RES_MEMORY]))
            if g:
                counts[g, zone[0, node]] += 1
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=synth.CONFIGS[3]["nodes"])
    ap.add_argument("--pods", type=int, default=synth.CONFIGS[3]["pods"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--zones", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=1, help="runs of each kind, alternating (the best of each is reported)")
    ap.add_argument("--kinds", default="ids_all_zero,all_grouped,tenth_grouped,one_group")
    ap.add_argument("--check-pods", type=int, default=128, help="lock-step oracle prefix of the all-grouped run (0 = off)")
    a = ap.parse_args()
    cl = synth.make_cluster(a.nodes, synth.BASE_SEED + 3)
    pods = synth.make_pods(a.pods, synth.BASE_SEED + 103)
    rng = np.random.default_rng(synth.BASE_SEED + 1504)
    # (maps, each group's map, its domains -- every zone --, its maxSkew)
    table = (np.arange(a.nodes)[None] % a.zones, np.ones(a.groups, np.int32), [(1 << a.zones) - 1] * a.groups,
             np.ones(a.groups, np.int32))
    all_ids = rng.integers(1, a.groups + 1, a.pods).astype(np.int32)
    kinds = {"ids_all_zero": np.zeros(a.pods, np.int32), "all_grouped": all_ids,
             "tenth_grouped": np.where(rng.random(a.pods) < 0.10, all_ids, 0).astype(np.int32),
             "one_group": np.ones(a.pods, np.int32)}
    kinds = {k: v for k, v in kinds.items() if k in a.kinds.split(",")}
    cfg = synth.config(a.nodes)
    runs = [{k: run(cfg, cl, table, pods, ids, a.steps, a.warmup) for k, ids in kinds.items()}
            for _ in range(max(1, a.repeats))]
    best = {k: max((r[k] for r in runs), key=lambda r: r["value"]) for k in kinds}
    out = {"workload": f"{a.nodes} nodes x {a.pods} pods (config-3 shape), {a.groups} spread domain groups of maxSkew 1 "
                       f"over {a.zones} zones",
           "unit": "pod-node evals/s", **best, "all_values": {k: [r[k]["value"] for r in runs] for k in kinds}}
    if a.check_pods and "all_grouped" in kinds:
        out["oracle_prefix_equal"] = oracle_prefix(cfg, cl, table, pods, all_ids, a.check_pods)
        out["oracle_prefix_pods"] = a.check_pods
    print(json.dumps(out))


if __name__ == "__main__":
    main()
