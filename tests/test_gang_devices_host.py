"""Gang runs with DeviceShare members (ke_set_gang_devices / ke_debug_gang_devices, ABI v14, additive), host side: the
switch and every refusal with it off and on, on a context without a device; plan_batches and plan_select with the
switch compiled alone with AddressSanitizer + UBSan (tests/gang/gang_ds_check.cpp, run as a program) against a Python
restatement on random layouts of members, DeviceShare pods and plain pods; the plan with the switch off; and the
reference alone on every input of test_gpu_gang_devices.py, with the claims each input is there for."""
import os
import subprocess

import numpy as np
import pytest

import gang_ds_ref as D
import gang_ref as G
from koordinator_amd import Evaluator, KoordEvalError, abi, synth
from test_gang_host import ask, ctx, plain, random_runs, refused, runs_text
from test_node_sets_host import code_of

HERE = os.path.dirname(os.path.abspath(__file__))
T0 = synth.T0


@pytest.fixture(scope="module")
def ds_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gang_ds") / "gang_ds_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "gang", "gang_ds_check.cpp")], check=True)
    return exe


# ---- the switch and the refusals (no device) ---------------------------------------------------------------------------
def ds_pods(n, seed=9721):
    pods = plain(n, seed)
    pods["device_requests"][:, D.GPU] = 1
    pods["has_other_requests"] = 1
    pods["gpu_ring_bus_bandwidth"] = abi.ABSENT
    return pods


def test_abi(lib):
    assert abi.ABI_VERSION == 14 and lib.ke_abi_version() == 14
    for name in ("ke_set_gang_devices", "ke_debug_gang_devices"):
        assert hasattr(lib, name), name
    ev = ctx()
    assert ev.debug_gang_devices() == dict(device_inverses=0, cuts_in_run=0, adopted=0, restored=0)


def test_the_switch_defaults_to_off_and_is_answered_without_a_device():
    ev = ctx()
    refused(ev, ds_pods(4), [(1, 2, 2)], "gangs: a DeviceShare member")
    ev.set_gang_devices(True)
    for call in (ev.schedule, ev.submit):  # every check passes: the call stops only at the missing device
        assert code_of(call, ds_pods(4), T0, gangs=[(1, 2, 2)]) == abi.ERR_NO_DEVICE
    ev.set_gang_devices(False)
    refused(ev, ds_pods(4), [(1, 2, 2)], "gangs: a DeviceShare member")


@pytest.mark.parametrize("on", [False, True])
def test_the_other_member_refusals_keep_their_texts(on):
    ds_pods = globals()["ds_pods"] if on else plain  # (off: a DeviceShare member is refused as such first)
    ev = ctx(B=7)
    ev.set_gang_devices(on)
    refused(ev, plain(10), [(1, 8, 8)], "gangs: a run longer than ke_config.pod_batch")
    import ds_hint_cases as dh
    hinted, hint = dh.pod_and_hints(next(c for c in dh.HINTS if c["kind"] == "handler"))
    hev = ctx()
    hev.set_gang_devices(on)
    hev.set_pod_device_hints([hint])
    refused(hev, [hinted, hinted], [(0, 2, 2)], "gangs: a member with device hints")
    ev = ctx()
    ev.set_gang_devices(on)
    cpuset = synth.make_cpuset_pods(6, synth.BASE_SEED + 9712, cpuset_fraction=1.0)
    refused(ev, cpuset, [(0, 3, 3)], "gangs: a cpuset member")
    numa = ds_pods(4)
    numa["numa_topology_policy"][2] = abi.NUMA_POLICY_SINGLE_NUMA_NODE
    refused(ev, numa, [(1, 3, 3)], "gangs: a NUMA-policy member")
    rsv = ds_pods(4)
    rsv["reservation_matched"][1] = abi.RSV_MATCHED
    refused(ev, rsv, [(0, 2, 2)], "gangs: a reservation-matched")
    cl = synth.make_cluster(8, synth.BASE_SEED + 9701)
    nev = ctx(cl=cl)
    nev.set_gang_devices(on)
    synth.load_numa(nev, synth.make_numa(cl, synth.BASE_SEED + 9713, policy_weights=(0.0, 0.4, 0.3, 0.3), no_zone_fraction=0.0))
    refused(nev, ds_pods(6), [(1, 3, 3)], "gangs: a context with NUMA topology policy state")
    sev = ctx(cfg=synth.config(8, global_node_offset=8), cl=cl)
    sev.set_gang_devices(on)
    refused(sev, ds_pods(6), [(1, 3, 3)], "gangs: a node-sharded context")


def test_refusals_of_a_deviceshare_member_with_the_switch_on():
    # an ElasticQuota tree: k_resolve_gang is not built for DeviceShare batches with quota
    I = G.make_input("quota-64")
    ev = Evaluator(I.cfg)
    I.load(ev)
    ev.set_gang_devices(True)
    pods = I.pods.copy()
    pods["device_requests"][2, D.GPU] = 1
    pods["has_other_requests"][2] = 1
    refused(ev, pods, I.runs, "gangs: a DeviceShare member together with an ElasticQuota tree")
    assert code_of(ev.schedule, I.pods, T0, gangs=I.runs) == abi.ERR_NO_DEVICE  # plain members beside the tree: as before
    # node sets or score tables: a DeviceShare pod in such a call is refused as before, member or not
    ev = ctx()
    ev.set_gang_devices(True)
    ev.node_sets_load([[0, 1, 2]], n_nodes=8)
    refused(ev, ds_pods(4), [(1, 2, 2)], "node sets: a DeviceShare pod in ke_schedule", node_sets=[1, 0, 0, 0])
    # a context without nodes plans every DeviceShare pod alone: a run would leave its batch
    ev = Evaluator(synth.config(8))
    ev.set_gang_devices(True)
    refused(ev, ds_pods(4), [(1, 2, 2)], "gangs: a DeviceShare member in a context without nodes")


# ---- the plan ------------------------------------------------------------------------------------------------------------
def plan_restated(P, B, ds, runs, on):
    """plan_batches over P pods (ds[p]: a DeviceShare pod; unsharded, no NUMA policies: they share batches) with `runs`:
    (cuts, [(pods, ds, cut, grouped)])."""
    start = {r[0]: r[1] for r in G.norm_runs(runs)}
    member = np.zeros(P, bool)
    for r in runs:
        member[r[0]:r[0] + r[1]] = True
    out, cuts, p = [], 0, 0
    while p < P:
        bp, has_ds, has_gang = 0, False, False
        while p + bp < P and bp < B:
            q = p + bp
            if bp > 0 and q in start and bp + start[q] > B:
                cuts += 1
                break
            if bp > 0 and not on and ((member[q] and has_ds) or (ds[q] and has_gang)):
                break
            has_ds, has_gang = has_ds or bool(ds[q]), has_gang or bool(member[q])
            bp += 1
        out.append((bp, int(has_ds), int(has_ds and bp > 1), int(has_gang)))
        p += bp
    return cuts, out


def random_layouts(seed, Bs=(7, 64)):
    rng = np.random.default_rng(D.S + seed)
    cases = []
    for B in Bs:
        for P in rng.integers(1, 400, 16):
            P = int(P)
            runs = random_runs(rng, P, B)
            ds = rng.random(P) < float(rng.choice([0.0, 0.2, 0.6]))
            cases.append((P, B, ds, runs))
    return cases


def plan_line(cmd, P, B, ds, runs, on=None):
    bits = "".join("1" if x else "0" for x in ds) or "-"
    return f"{cmd} {P} {B} {'' if on is None else int(on)} {bits} {runs_text(runs)}"


def test_plan_with_the_switch_on_random_layouts(ds_check):
    cases = random_layouts(1)
    cases += [(I.P, I.B, I.pods["device_requests"].any(axis=1), I.runs) for I in (D.make_input(n) for n in D.BUILDERS)]
    out = ask(ds_check, [plan_line("plan", P, B, ds, runs, True) for P, B, ds, runs in cases])
    mixed = 0
    for (P, B, ds, runs), line in zip(cases, out):
        v = [int(x) for x in line.split()]
        cuts, want = plan_restated(P, B, ds, runs, True)
        assert v[0] == cuts and v[1] == len(want) and v[2:] == [x for b in want for x in b], (P, B, runs)
        assert cuts == G.plan_cut(P, B, runs)[1] and [b[0] for b in want] == G.plan_cut(P, B, runs)[0]  # the cut rule alone
        mixed += sum(1 for b in want if b[1] and b[3])
    assert mixed > 40  # batches holding both a member and a DeviceShare pod occur often


def test_plan_with_the_switch_off_is_todays(ds_check):
    cases = random_layouts(2)
    out = ask(ds_check, [plan_line("off", P, B, ds, runs) for P, B, ds, runs in cases])
    assert out == ["1"] * len(cases)
    out = ask(ds_check, [plan_line("plan", P, B, ds, runs, False) for P, B, ds, runs in cases])
    split = 0
    for (P, B, ds, runs), line in zip(cases, out):
        v = [int(x) for x in line.split()]
        cuts, want = plan_restated(P, B, ds, runs, False)
        assert v[0] == cuts and v[2:] == [x for b in want for x in b], (P, B, runs)
        member = np.zeros(P, bool)
        for r in runs:
            member[r[0]:r[0] + r[1]] = True
        if not (member & ds).any():  # (a member that is a DeviceShare pod itself is refused before the plan)
            assert not any(b[1] and b[3] for b in want)
        split += len(want) - len(plan_restated(P, B, ds, runs, True)[1])
    assert split > 20  # today's rule ends batches the switch keeps whole


def test_select_plan_takes_extra_entries_for_an_exact_batch(ds_check):
    lines = [f"select {N} {pods} {extra}" for N in (1, 300, 100_000) for pods, extra in ((1, 0), (5, 3), (60, 4), (60, 9), (64, 1))]
    for line, out in zip(lines, ask(ds_check, lines)):
        _, N, pods, extra = (int(x) if x.isdigit() else x for x in line.split())
        L, kext, parts, is_sorted, default = (int(x) for x in out.split())
        # k_j + kext <= pods + kext <= KMAX: one key a lane still holds every list
        assert (L, kext, parts, is_sorted, default) == (64, min(extra, 64 - pods), 1, 0, 0), line


# ---- the reference alone, on every input of test_gpu_gang_devices.py ---------------------------------------------------
def members(I, i):
    r = I.runs[i]
    return slice(r[0], r[0] + r[1])


def results(name):
    I, res, o = D.reference(name)
    return I, (res if isinstance(res, list) else [res]), o


@pytest.mark.parametrize("name", list(D.BUILDERS))
def test_reference_is_consistent(name):
    I, res, o = results(name)
    for r in res:
        placed = r["chosen"] >= 0
        assert ((r["status"] == G.PLACED) | (r["status"] == G.WAITING) | (r["status"] == G.NONE))[placed].all()
        assert (r["tried"][r["status"] != G.ROLLED_BACK] == -1).all() and (r["tried"][r["status"] == G.ROLLED_BACK] >= 0).all()
        assert (r["score"][~placed] == -1).all() and (r["score"][placed] >= 0).all()
        assert r["counts"]["inverse_reserves"] == int((r["status"] == G.ROLLED_BACK).sum()) == len(r["rollbacks"])
        assert (r["minors"][~placed] == 0).all()
    # what the pods hold at the end is what the oracle's device cache gained: whole GPUs of the placed pods are full
    r = res[-1]
    pods = I.pods[-len(r["chosen"]):]
    for p in np.nonzero((r["chosen"] >= 0) & (pods["device_requests"][:, D.GPU] > 0))[0]:
        devs = o.node_state(int(r["chosen"][p]))[3]
        for d in devs:
            if d["type"] == abi.DEV_GPU and (int(r["minors"][p]) >> int(d["minor"])) & 1:
                assert d["has_used"].all() and d["used"][0] == 100, (name, p)


def test_inputs_contain_what_their_tests_claim():
    # every input but the one-node layouts at B = 64 (no room for a second member) rolls a run with devices back
    for name in D.BUILDERS:
        I, res, _ = results(name)
        inv = sum(1 for r in res for _, _, m in r["rollbacks"] if m)
        assert inv > 0 or name == "layout-1-64", name
    # layouts: the run of B - 1 is rolled back with at least five members on the larger clusters
    for name in ("layout-63-64", "layout-65-64", "layout-300-64", "layout-63-7", "layout-64-7", "layout-300-7"):
        I, (r,), _ = results(name)
        assert (r["status"][members(I, 2)] == G.ROLLED_BACK).sum() >= 5, name
    # n = 300: devices on two nodes in three; a DeviceShare pod never lands on a node without them
    I, (r,), _ = results("layout-300-64")
    assert all(I.devs[c] is not None for c, m in zip(r["chosen"], r["minors"]) if m)
    # kinds: a later pod lands on minors that a rolled-back member held, on the same node
    for name in (f"kind-{k}" for k in D.KINDS):
        I, (r,), _ = results(name)
        held = {(n, t) for _, n, m in r["rollbacks"] for t in range(48) if (m >> t) & 1}
        end = I.runs[0][0] + I.runs[0][1]
        after = {(int(r["chosen"][p]), t) for p in range(end, I.P) if r["chosen"][p] >= 0 for t in range(48) if (int(r["minors"][p]) >> t) & 1}
        assert held & after, name
    # shared kinds: two members on one minor
    for name in ("kind-shared-ratio", "kind-shared-bytes"):
        I, (r,), _ = results(name)
        taken = [(n, m) for _, n, m in r["rollbacks"]]
        assert len(set(taken)) < len(taken), name
    # GPU + RDMA: a member holds one minor of each type
    I, (r,), _ = results("kind-gpu-rdma")
    assert all(m & 0xFFFF and (m >> 16) & 0xFFFF for _, _, m in r["rollbacks"])
    # one node: the run's first member shares the non-member's minor; three inverses; the non-member's half stays and a
    # later pod takes the other half again: the minor is full at the end
    I, (r,), o = results("same-node")
    assert r["chosen"][0] == 0 and r["minors"][0] == 1
    assert [(p, m) for p, _, m in r["rollbacks"]] == [(1, 1), (2, 2), (3, 2)] and r["status"][4] == G.FAILED
    assert r["minors"][5] == 1 and (r["chosen"][5:8] == 0).all()
    # used keys present with value 0: a rolled-back member took that minor, and the host path dropped the keys -- they
    # come back only with the later pod that takes the minor again
    I, (r,), o = results("zero-keys")
    assert I.devs[0][0]["has_used"].all() and not I.devs[0][0]["used"].any()
    assert (0, 0, 1) in r["rollbacks"]
    probe = I.oracle()
    al = {}
    for p in range(4):
        c, _ = probe.schedule(I.pods[p:p + 1], T0)
        al[p] = (int(c[0]), probe.last_allocations(1)[0].copy())
    assert al[0][0] == 0 and al[0][1]["device_minors"] == 1
    probe.release(I.pods[0], al[0][1], abi.RELEASE_UNRESERVE)
    assert not probe.node_state(0)[3][0]["has_used"].any()  # dropped, though present before the Reserve
    # thresholds: every status occurs, and the last run is rolled back with both member kinds
    I, (r,), _ = results("thresholds")
    assert (np.bincount(r["status"], minlength=6) > 0).all()
    assert r["counts"] == dict(runs=7, rolled_back=2, inverse_reserves=3)
    # partition tables / topology beside default nodes: rolled-back members on both sorts of node
    I, (r,), _ = results("partition-topology")
    special = {i for i, (has, honor, _) in enumerate(I.parts) if has or honor} | {i for i in range(12)}
    nodes = {n for _, n, m in r["rollbacks"] if m}
    assert nodes & special and nodes - special
    # the cut inputs: the run fails after its second member at the earliest, with placed members to roll back
    for name in ("cut-in-run-64", "cut-in-run-7"):
        I, (r,), _ = results(name)
        first_failed = int(np.nonzero(r["status"] == G.FAILED)[0][0])
        assert first_failed - I.runs[0][0] >= 2 and len(r["rollbacks"]) >= 5, name
        assert I.cfg.deviceshare.strategy == abi.STRATEGY_MOST_ALLOCATED
    # the short-list inputs: in the state the failing last member sees, the first plain pod's two best nodes are nodes
    # the run filled; after the rollback the pod lands on neither
    for name in ("short-list-16-7", "short-list-16-8"):
        I, (r,), _ = results(name)
        last = I.runs[0][0] + I.runs[0][1] - 1
        held = {n for _, n, _ in r["rollbacks"]}
        assert r["status"][last] == G.FAILED and len(held) >= 2 and not I.pods["device_requests"][last + 1].any()
        o = I.oracle()
        for p in range(last):
            o.schedule(I.pods[p:p + 1], T0)
        t = o.eval(I.pods[last + 1:last + 2], T0)["total"][0].astype(np.int64)
        top = np.argsort(-t, kind="stable")[:3]
        assert set(top[:2].tolist()) <= held and t[top[1]] > t[top[2]], name
        assert r["chosen"][last + 1] >= 0 and int(r["chosen"][last + 1]) not in held, name
    # the mixed call: one rolled-back run between plain batches; the slices: a rolled-back run in each
    I, (r,), _ = results("mixed")
    assert r["counts"]["rolled_back"] == 1 and r["counts"]["inverse_reserves"] == 9
    I, rs, _ = results("slices")
    assert [x["counts"]["rolled_back"] for x in rs] == [1, 1]
