"""plan_batches' cut rule for spread domain term lists (koordinator_amd/csrc/ke_plan.h), compiled for
the host with g++ (tests/plan/dterms_plan_check.cpp) and compared with the restatement in spread_domain_terms.plan: a
batch ends before a pod one of whose term groups is a member group of an earlier pod of that batch -- no read after a
write inside a batch, batches as long as the rule and the size allow, grouped batches outside the pipelined runs; empty
lists give the plan without lists; {SKEW(g)} + {g} gives §4s's plan."""
import os
import subprocess

import numpy as np
import pytest

import spread_domains
from spread_domain_terms import from_domain_ids, make_input, plan

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dterms") / "dterms_plan_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(HERE, "plan", "dterms_plan_check.cpp")], check=True)
    return exe


def plans(exe, cases):
    """Per case (B, term groups per pod, members per pod): the three plans as ([(pods, grouped)], run_end)."""
    text = ""
    for B, tg, ml in cases:
        text += f"{B} {len(tg)} " + " ".join(f"{len(t)} {' '.join(map(str, t))} {len(m)} {' '.join(map(str, m))}"
                                              for t, m in zip(tg, ml)) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    out = []
    for line in r.stdout.splitlines():
        three = []
        for part in line.split("|")[1:]:
            b, runs = part.split("/")
            b = [int(x) for x in b.split()]
            three.append((list(zip(b[0::2], b[1::2])), [int(x) for x in runs.split()]))
        out.append(three)
    assert len(out) == len(cases)
    return out


def groups_of(terms):
    return [[t[0] for t in tl] for tl in terms]


def random_lists(rng, n, G, p_empty):
    tg, ml = [], []
    for _ in range(n):
        if rng.random() < p_empty:
            tg.append([]), ml.append([])
            continue
        tg.append([int(g) for g in rng.integers(1, G + 1, rng.integers(0, 5))])
        ml.append([int(g) for g in rng.choice(np.arange(1, G + 1), min(G, int(rng.integers(0, 5))), replace=False)])
    return tg, ml


def check_rule(B, tg, ml, batches):
    """No read after a write inside a batch; every batch is as long as the rule and B allow; marks."""
    assert sum(b for b, _ in batches) == len(tg)
    p = 0
    for b, grouped in batches:
        assert 1 <= b <= B
        written = set()
        for q in range(p, p + b):
            assert not (set(tg[q]) & written), (p, q)
            written |= set(ml[q])
        if p + b < len(tg) and b < B:  # maximal: the next pod reads a group this batch writes
            assert set(tg[p + b]) & written, (p, b)
        assert grouped == int(any(tg[q] or ml[q] for q in range(p, p + b)))
        p += b


def test_cut_rule_against_the_restatement(check):
    rng = np.random.default_rng(20261020)
    cases = []
    for B in (1, 2, 7, 64):
        for G, p_empty in ((2, 0.0), (5, 0.3), (40, 0.0), (40, 0.9)):
            tg, ml = random_lists(rng, 200, G, p_empty)
            cases.append((B, tg, ml))
    for name in ("P", "Q", "R"):
        c = make_input(name)
        cases += [(B, groups_of(c["dterms"]), c["dmembers"]) for B in (7, 64)]
    cuts = 0
    for (B, tg, ml), (with_lists, _, _) in zip(cases, plans(check, cases)):
        batches, run_end = with_lists
        assert [b for b, _ in batches] == plan([[(g,) for g in t] for t in tg], ml, B)
        check_rule(B, tg, ml, batches)
        cuts += sum(1 for b, _ in batches[:-1] if b < B)
        # a grouped batch is part of no pipelined run
        in_run = set()
        for b0, e in enumerate(run_end):
            in_run |= set(range(b0, e)) if e else set()
        assert not any(batches[b][1] for b in in_run)
    assert cuts > 100


def test_read_only_and_write_only_pods_share_full_batches(check):
    c = make_input("R")
    (with_lists, _, _), = plans(check, [(64, groups_of(c["dterms"]), c["dmembers"])])
    assert with_lists[0] == [(64, 1)] * 4 and not any(with_lists[1])
    # write after read and write after write stay together, a read after a write does not
    tg = [[1], [2], [], [], [3], [1]]
    ml = [[], [], [1], [1, 2], [4], []]
    (with_lists, _, _), = plans(check, [(64, tg, ml)])
    assert with_lists[0] == [(5, 1), (1, 1)]


def test_empty_lists_give_the_plan_without_lists(check):
    for B in (1, 7, 64):
        (with_lists, plain, ids), = plans(check, [(B, [[]] * 150, [[]] * 150)])
        assert with_lists == plain == ids
        assert all(not g for _, g in plain[0]) and any(plain[1])  # pipelined runs stay
    # a listed stretch behind a plain one: the plain batches keep their run
    tg = [[]] * 128 + [[1]] * 4
    ml = [[]] * 128 + [[1]] * 4
    (with_lists, plain, _), = plans(check, [(64, tg, ml)])
    assert with_lists[0] == [(64, 0), (64, 0), (1, 1), (1, 1), (1, 1), (1, 1)] and with_lists[1][0] == 2


@pytest.mark.parametrize("name", ["E", "F", "G", "H"])
def test_skew_on_the_own_group_is_the_domain_id_plan(check, name):
    c = from_domain_ids(spread_domains.make_input(name))
    for B in (7, 64):
        (with_lists, _, ids), = plans(check, [(B, groups_of(c["dterms"]), c["dmembers"])])
        assert with_lists == ids
        assert [b for b, _ in ids[0]] == spread_domains.plan(c["dids"], B)
