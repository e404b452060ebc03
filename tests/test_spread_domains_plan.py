"""The spread domain part of the host plan (ke_plan.h), compiled for the host with g++ (tests/plan/
domain_plan_check.cpp): a batch holds at most one pod of any spread domain group, every batch is as long as that
allows, a batch holding such a pod is marked and never inside a pipelined run, and the plan of a queue whose ids are
all zero is the one without ids."""
import os
import subprocess

import numpy as np
import pytest

from koordinator_amd import synth
from spread_domains import plan

HERE = os.path.dirname(os.path.abspath(__file__))
ALONE = 1 | 2 | 4  # PF_DS (ds_batch on: shares batches), PF_CPUSET, PF_DS_HINT as domain_plan_check.cpp reads them


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "domain_plan_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(HERE, "plan", "domain_plan_check.cpp")], check=True)
    return exe


def plans(exe, cases):
    """cases: (B, flags, dids) -> per case ((batches, run_end) with the ids, (batches, run_end) without)."""
    text = "".join(f"{B} {len(f)} " + " ".join(f"{a} {g}" for a, g in zip(f, dids)) + "\n" for B, f, dids in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.splitlines():
        halves = []
        for half in line.split("|"):
            b, runs = half.split("/")
            b = [int(x) for x in b.split()]
            halves.append(([tuple(b[i:i + 6]) for i in range(0, len(b), 6)], [int(x) for x in runs.split()]))
        out.append(tuple(halves))
    assert len(out) == len(cases)
    return out


def in_run(run_end):
    inside = np.zeros(len(run_end), bool)
    for b, e in enumerate(run_end):
        inside[b:e] = True  # (e = 0: not the first batch of a run)
    return inside


def test_the_issues_example(check):
    (bt, runs), _ = plans(check, [(64, [0] * 5, [1, 1, 2, 0, 1])])[0]
    assert [b[0] for b in bt] == [1, 3, 1] and all(b[5] for b in bt) and runs == [0, 0, 0]
    assert plan([1, 1, 2, 0, 1], 64) == [1, 3, 1]


def test_random_queues(check):
    rng = np.random.default_rng(synth.BASE_SEED + 9790)
    cases = []
    for B in (1, 2, 7, 64):
        for frac, groups in ((0.0, 1), (0.05, 3), (0.5, 2), (1.0, 9), (1.0, 200)):
            n = int(rng.integers(1, 400))
            flags = np.where(rng.random(n) < 0.05, rng.integers(1, 8, n), 0)
            dids = np.where(rng.random(n) < frac, rng.integers(1, groups + 1, n), 0)
            cases.append((B, flags.tolist(), dids.tolist()))
        n = int(rng.integers(100, 400))  # a plain queue: the Python restatement of the plan holds
        cases.append((B, [0] * n, np.where(rng.random(n) < 0.5, rng.integers(1, 6, n), 0).tolist()))
    some_cut = some_run = False
    for (B, flags, dids), ((bt, runs), (bt0, runs0)) in zip(cases, plans(check, cases)):
        inside, p = in_run(runs), 0
        alone = lambda q: bool(flags[q] & 6)  # noqa: E731  (a cpuset or hinted pod is alone in its batch)
        for k, b in enumerate(bt):
            ids = [g for g in dids[p:p + b[0]] if g]
            assert len(ids) == len(set(ids)), (B, k)  # no batch repeats a non-zero id
            assert bool(b[5]) == bool(ids), (B, k)
            assert not (ids and inside[k]), (B, k)  # a batch holding an id is outside runs
            e = p + b[0]
            # maximal: it ended at B, at the queue's end, at a repeat, or at a pod that must be alone (or is one)
            assert (b[0] == B or e == len(flags) or (dids[e] and dids[e] in ids) or alone(e) or alone(p)), (B, k)
            some_cut = some_cut or (b[0] < B and e < len(flags) and dids[e] in ids and not alone(e) and not alone(p))
            p = e
        assert p == len(flags)
        some_run = some_run or inside.any()
        if not any(dids):  # all ids zero: today's plan
            assert (bt, runs) == (bt0, runs0)
        if not any(flags):
            assert [b[0] for b in bt] == plan(dids, B), B
    assert some_cut and some_run
    # ids given but all zero
    (bt, runs), (bt0, runs0) = plans(check, [(7, [0, 1, 0, 2, 0, 0, 0, 0, 0, 4] * 5, [0] * 50)])[0]
    assert (bt, runs) == (bt0, runs0) and not any(b[5] for b in bt)


def test_plain_half_keeps_its_run(check):
    rng = np.random.default_rng(synth.BASE_SEED + 9791)
    dids = [0] * 128 + rng.integers(1, 4, 128).tolist()
    (bt, runs), _ = plans(check, [(64, [0] * 256, dids)])[0]
    assert [b[0] for b in bt[:2]] == [64, 64] and [b[5] for b in bt[:2]] == [0, 0]
    assert runs[0] == 2 and not any(runs[1:])
    assert all(b[5] for b in bt[2:]) and [b[0] for b in bt] == plan(dids, 64)
