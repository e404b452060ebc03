"""ke_preempt against the same algorithm on one CPU thread.

The bench's 50k-node cluster (BASELINE config 3) with its queue placed under the NodeResourcesFit profile.  Every placed
pod is listed as a resident, and synthetic residents bring the lists to a mean of 30 a node; their requests are part
of the nodes' Requested, which ends a little below Allocatable, so that a pending pod of 8 cores fits nowhere and
fits on many nodes once a few residents are gone.  8 quotas (half of them at their used limit), 200 PDBs.  Then 64 and
512 pending preemptors:
  (a) ke_preempt, with the resident table uploaded by the timed call (the table touched before each repeat) and
      without (the table unchanged since the call before);
  (b) the yardstick: the same steps 2-5 and the same pick as a single-threaded C++ restatement over the host copy of
      the same state, built -O2 by this tool.  It is given the classification and the other filters' verdict of every
      pair precomputed (ke_diagnose bitmaps of the context and of a twin context without NodeResourcesFit's Filter),
      so it times the victim selection alone -- which favours it.
3 warm-ups and 7 repeats each, min / median / max in ms; every device result is checked against the yardstick's.
Writes one JSON line, also to profiles/preempt/preempt_bench.json.
Usage: python tools/preempt_bench.py [--nodes 50000 --pods 100000 --preemptors 64 512 --repeats 7 --warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from koordinator_amd import Evaluator, abi, synth  # noqa: E402
from koordinator_amd.evaluator import unpack_node_sets  # noqa: E402

YARDSTICK = r"""
#include <cstdint>
#include <vector>
#include <algorithm>
// One thread, plain loops: SelectVictimsOnNode per (pod, node) and pickOneNodeForPreemption per pod.
// verdict[p*N+i]: 0 = not tried (unresolvable / error), 1 = tried, another filter fails, 2 = tried, the others pass
struct Key { uint64_t viol; int64_t hi; uint64_t sum; int64_t cnt; int64_t start; int64_t node; };
static bool better(const Key& a, const Key& b) {
  if (a.viol != b.viol) return a.viol < b.viol;
  if (a.hi != b.hi) return a.hi < b.hi;
  if (a.sum != b.sum) return a.sum < b.sum;
  if (a.cnt != b.cnt) return a.cnt < b.cnt;
  if (a.start != b.start) return a.start > b.start;
  return a.node < b.node;
}
extern "C" int yardstick(int N, int P, int fit_on, const int64_t* alloc, const int64_t* req, const int64_t* room,
                         const int32_t* off, const int64_t* r_cpu, const int64_t* r_mem, const int32_t* r_prio,
                         const int64_t* r_start, const int32_t* r_quota, const uint8_t* r_np, const int32_t* r_pdb,
                         const int64_t* r_uid, const int32_t* pdb_allowed, int n_pdb, const int64_t* p_req,
                         const int32_t* p_prio, const int32_t* p_quota, const int64_t* q_used, const int64_t* q_lim,
                         const uint8_t* q_lim_has, const uint8_t* q_max_has, int blocked_quota, const uint8_t* verdict,
                         int32_t* out, int cap, int64_t* victims) {
  std::vector<int32_t> budget(pdb_allowed, pdb_allowed + n_pdb), touched;
  std::vector<int> pot, order;
  std::vector<uint8_t> viol;
  std::vector<int64_t> vict, best_vict;
  for (int p = 0; p < P; p++) {
    int32_t* o = out + 8 * p;
    for (int k = 0; k < 8; k++) o[k] = 0;
    o[0] = -1;
    Key best{};
    bool have = false;
    const int64_t pc = p_req[2 * p], pm = p_req[2 * p + 1];
    const int q = p_quota[p];
    const int64_t* used0 = q_used + 2 * p;
    const int64_t* lim = q_lim + 2 * p;
    const uint8_t *lh = q_lim_has + 2 * p, *mh = q_max_has + 2 * p;
    for (int i = 0; i < N; i++) {
      const uint8_t v = verdict[(int64_t)p * N + i];
      if (v == 0) { o[4]++; continue; }
      pot.clear();
      for (int j = off[i]; j < off[i + 1]; j++)
        if (!r_np[j] && r_prio[j] < p_prio[p] && r_quota[j] == q && !(blocked_quota && r_quota[j] == blocked_quota)) pot.push_back(j);
      if (pot.empty()) { o[5]++; continue; }
      int64_t c0 = req[2 * i], c1 = req[2 * i + 1], rm = room[i], u0 = used0[0], u1 = used0[1];
      for (int j : pot) {
        c0 = std::max<int64_t>(0, c0 - r_cpu[j]), c1 = std::max<int64_t>(0, c1 - r_mem[j]), rm++;
        u0 = std::max<int64_t>(0, u0 - (mh[0] ? r_cpu[j] : 0)), u1 = std::max<int64_t>(0, u1 - (mh[1] ? r_mem[j] : 0));
      }
      auto fits = [&]() {
        if (v != 2) return false;
        if (!fit_on) return true;
        if (rm < 1) return false;
        if (pc > 0 && pc > alloc[2 * i] - c0) return false;
        if (pm > 0 && pm > alloc[2 * i + 1] - c1) return false;
        return true;
      };
      if (!fits()) { o[6]++; continue; }
      viol.assign(pot.size(), 0);
      touched.clear();
      for (size_t k = 0; k < pot.size(); k++)
        for (int s = 0; s < 2; s++) {
          const int x = r_pdb[2 * pot[k] + s];
          if (!x) continue;
          touched.push_back(x - 1);
          if (--budget[x - 1] < 0) viol[k] = 1;
        }
      for (int x : touched) budget[x] = pdb_allowed[x];
      order.clear();
      for (size_t k = 0; k < pot.size(); k++) if (viol[k]) order.push_back((int)k);
      const size_t n_violating = order.size();
      for (size_t k = 0; k < pot.size(); k++) if (!viol[k]) order.push_back((int)k);
      vict.clear();
      int64_t nviol = 0, hi = INT32_MIN, start = INT64_MAX;
      uint64_t sum = 0;
      bool err = false;
      for (size_t t = 0; t < order.size() && !err; t++) {
        const int j = pot[order[t]];
        const int64_t q0 = mh[0] ? r_cpu[j] : 0, q1 = mh[1] ? r_mem[j] : 0;
        auto remove = [&]() {
          c0 = std::max<int64_t>(0, c0 - r_cpu[j]), c1 = std::max<int64_t>(0, c1 - r_mem[j]), rm++;
          u0 = std::max<int64_t>(0, u0 - q0), u1 = std::max<int64_t>(0, u1 - q1);
          vict.push_back(r_uid[j]);
          sum += (uint64_t)((int64_t)r_prio[j] + 2147483649LL);
          if (r_prio[j] > hi) hi = r_prio[j], start = r_start[j];
          else if (r_prio[j] == hi) start = std::min(start, r_start[j]);
        };
        c0 += r_cpu[j], c1 += r_mem[j], rm--, u0 += q0, u1 += q1;
        const bool fit = fits();
        if (!fit) { remove(); nviol += t < n_violating; }
        const bool ok = q == 0 || (!(lh[0] && u0 + (mh[0] ? pc : 0) > lim[0]) && !(lh[1] && u1 + (mh[1] ? pm : 0) > lim[1]));
        if (!ok) { if (!fit) err = true; else remove(); }
      }
      if (err) { o[7]++; continue; }
      o[3]++;
      const Key key{(uint64_t)nviol, hi, sum, (int64_t)vict.size(), start, i};
      if (!have || better(key, best)) best = key, have = true, best_vict = vict;
    }
    if (have) {
      o[0] = (int32_t)best.node, o[1] = (int32_t)best.cnt, o[2] = (int32_t)best.viol;
      for (int k = 0; k < cap; k++) victims[(int64_t)p * cap + k] = k < (int)best_vict.size() ? best_vict[k] : 0;
    } else {
      for (int k = 0; k < cap; k++) victims[(int64_t)p * cap + k] = 0;
    }
  }
  return 0;
}
"""


def build_yardstick():
    d = tempfile.mkdtemp(prefix="preempt_yardstick_")
    src, so = os.path.join(d, "yardstick.cpp"), os.path.join(d, "yardstick.so")
    with open(src, "w") as f:
        f.write(YARDSTICK)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.yardstick.restype = C.c_int
    return lib


def series(fn, warmup, repeats, before=None):
    for _ in range(warmup):
        if before:
            before()
        fn()
    ms = []
    for _ in range(repeats):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"min": min(ms), "median": float(np.median(ms)), "max": max(ms), "all": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=synth.CONFIGS[3]["nodes"])
    ap.add_argument("--pods", type=int, default=synth.CONFIGS[3]["pods"])
    ap.add_argument("--preemptors", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mean-residents", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preempt", "preempt_bench.json"))
    a = ap.parse_args()
    N, now = a.nodes, int(synth.T0)
    rng = np.random.default_rng(synth.BASE_SEED + 1700)
    cl = synth.make_cluster(N, synth.BASE_SEED + 3)
    queue = synth.add_fit_defaults(synth.make_pods(a.pods, synth.BASE_SEED + 103))
    cfg = synth.fit_config(synth.config(N))
    twin_cfg = type(cfg).from_buffer_copy(cfg)
    twin_cfg.fit.filter = 0
    ev, twin = Evaluator(cfg), Evaluator(twin_cfg)
    synth.load_into(ev, cl), synth.load_into(twin, cl)
    chosen = np.concatenate([ev.schedule(queue[s:s + max(1, a.pods // 20)], now)[0]
                             for s in range(0, a.pods, max(1, a.pods // 20))])
    placed = np.nonzero(chosen >= 0)[0]
    twin.assign_bulk(chosen[placed].astype(np.int32), queue[placed], np.full(len(placed), now, np.int64))

    # ---- residents: the placed pods, then synthetic ones whose requests fill the node to a little below Allocatable
    alloc = np.ascontiguousarray(cl.nodes["allocatable"][:, :2], np.int64)
    req = np.zeros((N, 2), np.int64)
    for i in range(N):
        r2, nz = (C.c_int64 * 2)(), (C.c_int64 * 2)()
        ev._check(ev.lib.ke_node_info_requested(ev.h, i, r2, nz))
        req[i] = (r2[0], r2[1])
    per_node = np.bincount(chosen[placed], minlength=N)
    n_syn = np.maximum(1, rng.poisson(max(1, a.mean_residents - len(placed) / N), N))
    slack = np.stack([rng.integers(0, 5, N) * 1000, rng.integers(0, 9, N) * synth.GI], 1)
    fill = np.maximum(0, alloc - slack - req)
    total = int(len(placed) + n_syn.sum())
    recs = np.zeros(total, abi.RESIDENT_POD_DTYPE)
    node_of = np.concatenate([chosen[placed], np.repeat(np.arange(N), n_syn)])
    recs["requests"][:len(placed), 0] = queue["requests"][placed, abi.RES_CPU]
    recs["requests"][:len(placed), 1] = queue["requests"][placed, abi.RES_MEMORY]
    recs["requests"][len(placed):, 0] = np.repeat(fill[:, 0] // n_syn, n_syn)
    recs["requests"][len(placed):, 1] = np.repeat(fill[:, 1] // n_syn, n_syn)
    recs["uid"] = 50_000_000 + np.arange(total)
    recs["priority"] = rng.choice([100, 1000, 5000, 9000], total)
    recs["start_ns"] = now - rng.integers(1, 500, total) * 60 * synth.NS
    recs["quota"] = rng.integers(2, 10, total)        # the 8 leaves of the tree below (index 0 is their parent)
    recs["non_preemptible"] = rng.random(total) < 0.1
    with_pdb = rng.random(total) < 0.3
    recs["n_pdb"] = with_pdb
    recs["pdb"][:, 0] = np.where(with_pdb, rng.integers(1, 201, total), 0)
    order = np.argsort(node_of, kind="stable")
    recs, node_of = np.ascontiguousarray(recs[order]), node_of[order]
    off = np.zeros(N + 1, np.int32)
    off[1:] = np.cumsum(np.bincount(node_of, minlength=N))
    new_req = req + (fill // n_syn[:, None]) * n_syn[:, None]
    for h in (ev, twin):
        for i in range(N):
            h.set_requested(i, int(new_req[i, 0]), int(new_req[i, 1]))
    pdbs = rng.integers(0, 4, 200).astype(np.int32)
    qa = synth.make_quota_tree(synth.BASE_SEED + 1701, n_leaves=8, fanout=8, total_cpu=40_000_000, total_mem=160_000 * synth.GI)
    for leaf in range(1, 9):
        qa[leaf]["used"] = qa[leaf]["max"] if leaf % 2 == 0 else (qa[leaf]["max"][0] // 2, qa[leaf]["max"][1] // 2)
    ev.quotas_load(synth.quota_args(40_000_000, 160_000 * synth.GI, runtime=False), qa)
    ev._check(ev.lib.ke_resident_pods_load(ev.h, N, abi.ptr(off), abi.ptr(recs)))
    ev.pdbs_load(pdbs)
    # the table in list order, for the yardstick
    host = np.concatenate([ev.resident_pods_get(i) for i in range(N)]) if total else recs
    assert len(host) == total
    room = (cl.nodes["allowed_pods"].astype(np.int64) - cl.nodes["pod_count"] - per_node).astype(np.int64)
    ylib = build_yardstick()
    y_res = [np.ascontiguousarray(x) for x in (
        host["requests"][:, 0], host["requests"][:, 1], host["priority"].astype(np.int32), host["start_ns"],
        host["quota"].astype(np.int32), host["non_preemptible"].astype(np.uint8), host["pdb"].astype(np.int32), host["uid"])]

    out = {"workload": f"{N} nodes, {a.pods} pods of the config-3 queue placed ({len(placed)} on a node), NodeResourcesFit "
                       f"Filter on; {total} resident pods (mean {total / N:.1f} a node), 8 quotas, 200 PDBs",
           "unit": "ms wall per call", "repeats": a.repeats, "warmup": a.warmup, "preemptors": {}}
    ok = True
    cap, wpp = 16, (N + 63) // 64
    for P in a.preemptors:
        pods = synth.make_pods(P, synth.BASE_SEED + 1702, key_base=9_000_000_000)
        for f in ("requests", "limits"):
            pods[f][:] = 0
            pods[f][:, abi.RES_CPU], pods[f][:, abi.RES_MEMORY] = 8000, 16 * synth.GI
        pods["priority_class"], pods["qos_class"], pods["is_daemonset"] = abi.PRIORITY_PROD, abi.QOS_LS, 0
        pods["quota"] = rng.integers(2, 10, P)
        pri = rng.choice([2000, 6000, 10000], P).astype(np.int32)
        # the pairs' classification and the other filters' verdict, precomputed for the yardstick
        real, other = ev.diagnose(pods, now, bitmaps=True), twin.diagnose(pods, now, bitmaps=True)
        verdict = np.where(real["unresolvable"], 0, np.where(other["feasible"], 2, 1)).astype(np.uint8)
        q_used, q_lim = np.zeros((P, 2), np.int64), np.zeros((P, 2), np.int64)
        q_lh, q_mh = np.zeros((P, 2), np.uint8), np.zeros((P, 2), np.uint8)
        states = {q: ev.quota_state(q - 1) for q in set(int(x) for x in pods["quota"])}
        for p in range(P):
            st, q = states[int(pods["quota"][p])], int(pods["quota"][p])
            q_used[p], q_lim[p], q_lh[p], q_mh[p] = st["used"], st["limit"], st["limit_has"], qa["has_max"][q - 1]
        p_req = np.ascontiguousarray(np.stack([pods["requests"][:, abi.RES_CPU], pods["requests"][:, abi.RES_MEMORY]], 1))
        p_quota = np.ascontiguousarray(pods["quota"], np.int32)
        y_out, y_vict = np.zeros((P, 8), np.int32), np.zeros((P, cap), np.int64)

        def yard():
            ylib.yardstick(N, P, 1, abi.ptr(alloc), abi.ptr(np.ascontiguousarray(new_req)), abi.ptr(room), abi.ptr(off),
                           *[abi.ptr(x) for x in y_res], abi.ptr(pdbs), len(pdbs), abi.ptr(p_req), abi.ptr(pri),
                           abi.ptr(p_quota), abi.ptr(q_used), abi.ptr(q_lim), abi.ptr(q_lh), abi.ptr(q_mh), 0,
                           abi.ptr(verdict), abi.ptr(y_out), cap, abi.ptr(y_vict))

        rec, vic = np.zeros(P, abi.PREEMPTION_DTYPE), np.zeros((P, cap), np.int64)

        def device():
            ev._check(ev.lib.ke_preempt(ev.h, P, abi.ptr(pods), abi.ptr(pri), now, None, abi.ptr(rec), cap, abi.ptr(vic),
                                        wpp, None))

        def touch():  # the table changed since the last call: the next one uploads it whole
            ev.resident_pod_add(0, np.zeros((), abi.RESIDENT_POD_DTYPE))
            ev.resident_pod_remove(0, 0)

        r = {"ke_preempt_with_table_upload": series(device, a.warmup, a.repeats, before=touch),
             "ke_preempt": series(device, a.warmup, a.repeats),
             "yardstick_one_cpu_thread": series(yard, a.warmup, a.repeats)}
        names = ("node", "n_victims", "n_pdb_violations", "n_candidates", "n_skipped", "n_no_victims", "n_unfit", "n_error")
        same = all(np.array_equal(rec[k], y_out[:, j]) for j, k in enumerate(names)) and np.array_equal(vic, y_vict)
        r["device_equals_the_yardstick"] = bool(same)
        ok = ok and same
        r["fit_nowhere"] = bool((real["n_feasible"] == 0).all())
        r["classes"] = {k: int(rec[k].sum()) for k in names[3:]}
        r["picked"], r["victims_mean"] = int((rec["node"] >= 0).sum()), float(rec["n_victims"].mean())
        base = r["yardstick_one_cpu_thread"]["min"]
        r["condition_slowest_device_repeat_faster_than_fastest_yardstick"] = bool(
            max(r["ke_preempt"]["max"], r["ke_preempt_with_table_upload"]["max"]) < base)
        r["speedup_median"] = {k: r["yardstick_one_cpu_thread"]["median"] / r[k]["median"]
                               for k in ("ke_preempt", "ke_preempt_with_table_upload")}
        out["preemptors"][str(P)] = r
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    ev.close(), twin.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
