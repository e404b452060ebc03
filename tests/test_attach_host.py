"""A call's per-pod attachments (koordinator_amd/csrc/ke_attach.h: the kernel mode of a call, the staging block behind
its pod records, the host's share of the Reserves) compiled for the host with g++ (tests/plan/attach_check.cpp), once
plainly and once under AddressSanitizer + UBSan, and compared with restatements of the rules here."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NS_SETS, NS_SCORES, NS_GROUPS, NS_DOMAINS, NS_TERMS = 1, 2, 3, 4, 5
SAN = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def attach_check(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attach") / ("attach_check_" + request.param))
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *(SAN if request.param == "sanitized" else ()),
                    "-o", exe, os.path.join(HERE, "plan", "attach_check.cpp")], check=True)
    return exe


def run(exe, mode, text=""):
    r = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.splitlines()


# ---- the rules, restated ---------------------------------------------------------------------------------------------
def call_ns(sets, scores, groups, domains, terms):
    return (NS_TERMS if terms else NS_DOMAINS if domains else NS_GROUPS if groups else NS_SCORES if scores
            else NS_SETS if sets else 0)


def batch_ns(grouped, sets, scores, groups, domains, terms):
    if not grouped:
        return NS_SCORES if scores else NS_SETS if sets else 0
    return NS_TERMS if terms else NS_DOMAINS if domains else NS_GROUPS


def staging_block(n_pods, sets, scores, groups, domains, terms):
    """A later kind brings the earlier ones' words with it: (ids, groups, domains, terms, total) in int32 words."""
    st = bool(terms)
    sd = st or bool(domains)
    sg = sd or bool(groups)
    ns = sg or bool(sets) or bool(scores)
    total = n_pods * (int(ns) + int(sg) + int(sd) + 8 * int(st))
    return (0 if ns else -1, n_pods if sg else -1, 2 * n_pods if sd else -1, 3 * n_pods if st else -1, total)


def test_modes_and_layout_of_every_combination(attach_check):
    lines = run(attach_check, "modes")
    seen = set()
    for line in lines:
        key, modes, layout, plan = ([int(x) for x in part.split()] for part in line.split("|"))
        sets, scores, domains, gt, n = key
        groups, terms = gt == 1, gt == 2
        seen.add(tuple(key))
        k = (sets, scores, groups, domains, terms)
        assert modes == [call_ns(*k), call_ns(sets, 0, groups, domains, terms), batch_ns(False, *k), batch_ns(True, *k)], key
        assert tuple(layout) == staging_block(n, *k), key
        # plan_batches' marks: the term marks stand in for the group ids
        assert plan == [gt, domains], key
    assert seen == {(s, c, d, gt, n) for s in (0, 1) for c in (0, 1) for d in (0, 1) for gt in (0, 1, 2) for n in (0, 1, 5)}
    assert len(lines) == 24 * 3


def test_apply_placements(attach_check):
    NONE = [0] * 8
    steps = [
        # a plain increment: pod 0 (group 1) on node 0, pod 1 (group 2) on node 3, pod 2 without a group
        ("groups 3  1 2 0  0 3 1", [1, 0, 0, 0, 0, 0, 0, 1], (0, 0, 0)),
        # chosen = -1, and a node index at sg_stride: nothing moves
        ("groups 2  1 2  -1 4", [1, 0, 0, 0, 0, 0, 0, 1], (0, 0, 0)),
        # an id beyond the loaded groups: nothing moves
        ("groups 1  3  1", [1, 0, 0, 0, 0, 0, 0, 1], (0, 0, 0)),
        ("set 1 2 65534", [1, 0, 65534, 0, 0, 0, 0, 1], (0, 0, 0)),
        # members saturate at 65535: group 1 on node 2 goes 65534 -> 65535 and stays, group 2 counts on
        ("terms 1  1 2  2", [1, 0, 65535, 0, 0, 0, 1, 1], (0, 0, 0)),
        ("terms 1  1 2  2", [1, 0, 65535, 0, 0, 0, 2, 1], (0, 0, 0)),
        # a record without members, an unplaced pod, a node at sg_stride
        ("terms 3  0 0  1 0  2 0  1 -1 4", [1, 0, 65535, 0, 0, 0, 2, 1], (0, 0, 0)),
        # domains through the group's map: node 0 -> domain 0, node 1 -> domain 1, node 3 -> domain 0
        ("domains 3  1 1 1  0 1 3", [1, 0, 65535, 0, 0, 0, 2, 1], (2, 1, 0)),
        # a node whose domain is KE_DOMAIN_NONE, chosen = -1, a node index at sd_stride, id 0, an id beyond the groups
        ("domains 5  1 1 1 0 2  2 -1 4 0 0", [1, 0, 65535, 0, 0, 0, 2, 1], (2, 1, 0)),
    ]
    assert steps[0][1] != NONE
    lines = run(attach_check, "apply", "\n".join(s[0] for s in steps) + "\n")
    assert len(lines) == len(steps)
    for (cmd, sg, sd), line in zip(steps, lines):
        f = line.split()
        assert f[0] == "sg" and f[9] == "sd", line
        assert [int(x) for x in f[1:9]] == sg, cmd
        assert tuple(int(x) for x in f[10:13]) == sd, cmd


def test_slot_take(attach_check):
    """take(): nothing staged -> false and an empty call vector; staged -> the ids move to the call, the staging is
    empty and off; the next take finds nothing and clears the call vector."""
    assert run(attach_check, "apply", "slot\n") == ["slot 0 1 1 3 0 0 0 0"]
