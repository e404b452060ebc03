"""The spread group part of the host plan (ke_plan.h), compiled for the host with g++ (tests/plan/
spread_plan_check.cpp): a batch holding a grouped pod is marked and never inside a pipelined run, and the batches
and runs of a queue without grouped pods are what they are without group ids."""
import os
import subprocess

import numpy as np
import pytest

from koordinator_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "spread_plan_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(HERE, "plan", "spread_plan_check.cpp")], check=True)
    return exe


def plans(exe, cases):
    """cases: (B, flags, gids) -> per case ((batches, run_end) with the ids, (batches, run_end) without)."""
    text = "".join(f"{B} {len(f)} " + " ".join(f"{a} {g}" for a, g in zip(f, gids)) + "\n" for B, f, gids in cases)
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


def test_grouped_batches_are_marked_and_outside_runs(check):
    rng = np.random.default_rng(synth.BASE_SEED + 9650)
    cases = []
    for B in (1, 2, 7, 64):
        for frac in (0.0, 0.02, 0.3, 1.0):
            n = int(rng.integers(1, 400))
            flags = np.where(rng.random(n) < 0.05, rng.integers(1, 8, n), 0)
            gids = np.where(rng.random(n) < frac, rng.integers(1, 9, n), 0)
            cases.append((B, flags.tolist(), gids.tolist()))
    # the mixed queue of the GPU test: 128 plain pods, then 128 grouped ones
    cases.append((64, [0] * 256, [0] * 128 + [3] * 128))
    some_grouped = some_run = False
    for (B, flags, gids), ((bt, runs), (bt0, runs0)) in zip(cases, plans(check, cases)):
        # the segmentation does not depend on the ids
        assert [b[:5] for b in bt] == [b[:5] for b in bt0]
        assert not any(b[5] for b in bt0)
        inside, p = in_run(runs), 0
        for k, b in enumerate(bt):
            want = any(g != 0 for g in gids[p:p + b[0]])
            assert bool(b[5]) == want, (B, k)
            assert not (want and inside[k]), (B, k)  # a grouped batch is never inside a run
            p += b[0]
        assert p == len(flags)
        some_grouped = some_grouped or any(b[5] for b in bt)
        some_run = some_run or inside.any()
        if not any(gids):  # no grouped pod: the plan without ids
            assert (bt, runs) == (bt0, runs0)
    assert some_grouped and some_run
    (bt, runs), _ = plans(check, cases[-1:])[0]
    assert [b[5] for b in bt] == [0, 0, 1, 1] and runs == [2, 0, 0, 0]  # the plain half still runs pipelined


def test_runs_between_grouped_batches_are_those_of_the_plain_stretches(check):
    # plain stretches of >= 2 batches on either side of a grouped batch form runs of their own
    gids = [0] * 20 + [1] + [0] * 9 + [0] * 30
    (bt, runs), (bt0, runs0) = plans(check, [(10, [0] * 60, gids)])[0]
    assert [b[0] for b in bt] == [10] * 6 and [b[5] for b in bt] == [0, 0, 1, 0, 0, 0]
    assert runs == [2, 0, 0, 6, 0, 0] and runs0 == [6, 0, 0, 0, 0, 0]
