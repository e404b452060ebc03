"""ke_diagnose's host side, no device needed: the reason tables (ke_reason_message / ke_reason_plugin), the fold of
raw tallies into a ke_pod_diagnosis (koordinator_amd/csrc/ke_diag.h compiled alone with g++, tests/diag/
diag_check.cpp) and the call's admission on a context without a device."""
import os
import re
import subprocess

import numpy as np
import pytest

from koordinator_amd import Evaluator, KoordEvalError, abi, reason_message, reason_plugin, synth

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "koord_eval.h")
T0 = synth.T0


def header_reasons():
    text = open(HEADER).read()
    return {name: int(v) for name, v in re.findall(r"#define (KE_REASON_\w+) (\d+)", text)}


# ---- the tables ------------------------------------------------------------------------------------------------------
def test_every_reason_has_a_message(lib):
    reasons = header_reasons()
    assert len(reasons) > 40 and reasons["KE_REASON_NONE"] == 0 and max(reasons.values()) < abi.DIAG_REASONS
    for name, r in reasons.items():
        if r:
            assert reason_message(r), name
    for r in (127, -1, 200):
        assert lib.ke_reason_message(r) == b""
    assert lib.ke_reason_message(0) is not None


def test_loadaware_messages_equal_the_header_quotes():
    assert reason_message(1) == "node(s) nodeMetric expired"
    assert reason_message(2) == "node(s) cpu usage exceed threshold"
    assert reason_message(4) == "node(s) cpu aggregated usage exceed threshold"
    assert reason_message(16) == "Insufficient amplified cpu"
    assert reason_message(67) == "Insufficient <resource name>"
    assert reason_message(abi.REASON_NODE_SET) == "node(s) didn't match the pod's node set"
    # every message the header quotes in full beside its define is the one returned
    text = open(HEADER).read()
    quoted = re.findall(r'#define (KE_REASON_\w+) (\d+)\s*/\* "([^"]+)"', text)
    assert len(quoted) >= 15
    for name, r, msg in quoted:
        if "..." not in msg and "<" not in msg:
            assert reason_message(int(r)) == msg, name


def test_reason_plugin_ranges():
    ranges = ((1, 15, abi.PLUGIN_LOADAWARE), (16, 31, abi.PLUGIN_NODENUMARESOURCE), (32, 49, abi.PLUGIN_DEVICESHARE),
              (50, 63, abi.PLUGIN_RESERVATION), (64, 95, abi.PLUGIN_NODERESOURCESFIT), (96, 96, abi.PLUGIN_NODE_SET))
    want = {r: bit for lo, hi, bit in ranges for r in range(lo, hi + 1)}
    for r in range(-3, 260):
        assert reason_plugin(r) == want.get(r, 0), r
    assert reason_plugin(0) == 0
    assert [abi.PLUGIN_LOADAWARE, abi.PLUGIN_NODENUMARESOURCE, abi.PLUGIN_DEVICESHARE, abi.PLUGIN_RESERVATION,
            abi.PLUGIN_NODERESOURCESFIT, abi.PLUGIN_NODE_SET] == [1, 2, 4, 8, 16, 32]
    for name, r in header_reasons().items():
        if r:
            assert reason_plugin(r) != 0, name


def test_struct_is_in_the_abi_list(lib):
    assert abi.STRUCTS[-1] is abi.PodDiagnosis
    sizes = (abi.i32 * len(abi.STRUCTS))()
    assert lib.ke_abi_struct_sizes(sizes, len(abi.STRUCTS)) == len(abi.STRUCTS)
    assert sizes[len(abi.STRUCTS) - 1] == 32 + 4 * abi.DIAG_REASONS
    assert lib.ke_abi_version() == 14


# ---- the fold (ke_diag.h alone) ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def diag_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("diag") / "diag_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(HERE, "diag", "diag_check.cpp")], check=True)
    return exe


def run(exe, mode, text=""):
    r = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.splitlines()


def test_fold_of_hand_made_tallies(diag_check):
    lines = [
        # n_slots absent feasible unsched unres error  reason:count ...
        "100 4 10 70 16 0  0:10 2:40 3:30 32:10 96:6",         # LoadAware + DeviceShare + node set
        "50 0 0 50 0 0  65:20 66:25 67:5",                     # NodeResourcesFit alone
        "64 1 3 20 38 2  0:5 1:2 19:18 23:38",                 # an error node counts under reason 0
        "7 7 0 0 0 0",                                         # every slot empty
        "0 0 0 0 0 0",                                         # no node
        "10 0 4 6 0 0  0:4 52:6",                              # Reservation
    ]
    out = [[int(x) for x in line.split()] for line in run(diag_check, "fold", "\n".join(lines) + "\n")]
    L, N, D, R, F, S = (abi.PLUGIN_LOADAWARE, abi.PLUGIN_NODENUMARESOURCE, abi.PLUGIN_DEVICESHARE,
                        abi.PLUGIN_RESERVATION, abi.PLUGIN_NODERESOURCESFIT, abi.PLUGIN_NODE_SET)
    #            ok n_nodes absent feas unsch unres err plugins reason0 rest
    assert out == [[1, 96, 4, 10, 70, 16, 0, L | D | S, 10, 86],
                   [1, 50, 0, 0, 50, 0, 0, F, 0, 50],
                   [1, 63, 1, 3, 20, 38, 2, L | N, 5, 58],
                   [1, 0, 7, 0, 0, 0, 0, 0, 0, 0],
                   [1, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                   [1, 10, 0, 4, 6, 0, 0, R, 4, 6]]
    for ok, n_nodes, absent, feas, unsch, unres, err, _, r0, rest in out:  # the four invariants
        assert ok == 1 and feas + unsch + unres + err == n_nodes and rest == unsch + unres and r0 == feas + err
    for (slots, row) in zip((100, 50, 64, 7, 0, 10), out):
        assert row[1] + row[2] == slots


def test_fold_refuses_tallies_that_do_not_add_up(diag_check):
    bad = ["100 4 10 70 16 0  0:10 2:40 3:30 32:10",   # six failing nodes without a reason
           "100 5 10 70 16 0  0:10 2:40 3:30 32:10 96:6",  # a slot too many
           "100 4 10 70 16 0  0:9 2:40 3:30 32:10 96:6"]   # reason 0 short of feasible + error
    assert [line.split()[0] for line in run(diag_check, "fold", "\n".join(bad) + "\n")] == ["0", "0", "0"]


def test_tables_of_the_header_alone_equal_the_library(diag_check, lib):
    rows = [line.split(" ", 2) for line in run(diag_check, "tables")]
    assert len(rows) == abi.DIAG_REASONS
    for r, plugin, msg in rows:
        assert int(plugin) == lib.ke_reason_plugin(int(r)) and msg == lib.ke_reason_message(int(r)).decode(), r


# ---- admission on a context without a device -------------------------------------------------------------------------
def ctx(n=70, **kw):
    cl = synth.make_cluster(n, synth.BASE_SEED + 9301)
    ev = Evaluator(synth.config(n, **kw))
    synth.load_into(ev, cl)
    return ev


def call(ev, pods, out="rec", wpp=None, bitmap=True, ids=None):
    pods = np.ascontiguousarray(pods)
    if ids is not None:
        ev.pod_node_sets(ids)
    rec = np.zeros(max(len(pods), 1), abi.POD_DIAGNOSIS_DTYPE)
    wpp = (ev.num_nodes + 63) // 64 if wpp is None else wpp
    words = np.zeros((max(len(pods), 1), max(wpp, 1)), np.uint64)
    rc = ev.lib.ke_diagnose(ev.h, len(pods), abi.ptr(pods), int(T0), abi.ptr(rec) if out else None, wpp,
                            None, abi.ptr(words) if bitmap else None, None)
    return rc, ev.lib.ke_last_error().decode()


def ids_gone(ev, pods):
    """Staged set ids of len(pods) pods would refuse a call of one pod fewer with KE_ERR_INVALID."""
    rc, msg = call(ev, pods[:-1])
    return rc != abi.ERR_INVALID, (rc, msg)


def test_admission_order_without_a_device(lib):
    ev = ctx()
    assert ev.num_nodes == 70  # two bitmap words a pod
    ev.node_sets_load(np.ones((2, 70), bool))
    pods = synth.make_pods(3, synth.BASE_SEED + 9302)
    ids = [1, 2, 0]
    last = abi.OK if lib.ke_device_available() else abi.ERR_NO_DEVICE
    assert lib.ke_diagnose(None, 0, None, 0, None, 0, None, None, None) == abi.ERR_INVALID
    # a null out
    rc, msg = call(ev, pods, out=None, ids=ids)
    assert rc == abi.ERR_INVALID and "out" in msg
    assert ids_gone(ev, pods)[0]
    # a bitmap with words_per_pod one too small; without a bitmap the same words_per_pod is ignored
    rc, msg = call(ev, pods, wpp=1, ids=ids)
    assert rc == abi.ERR_INVALID and "words_per_pod" in msg
    assert ids_gone(ev, pods)[0]
    assert call(ev, pods, wpp=1, bitmap=False)[0] == last
    # a reservation-matched pod
    matched = pods.copy()
    matched["reservation_matched"][1] = abi.RSV_MATCHED
    for with_ids in (ids, None):
        rc, msg = call(ev, matched, ids=with_ids)
        assert rc == abi.ERR_UNSUPPORTED, msg
        assert ids_gone(ev, pods)[0]
    # a node-sharded context
    sharded = ctx(global_node_offset=70)
    sharded.node_sets_load(np.ones((2, 70), bool))
    for with_ids in (ids, None):
        rc, msg = call(sharded, pods, ids=with_ids)
        assert rc == abi.ERR_UNSUPPORTED and "node-sharded" in msg
        assert ids_gone(sharded, pods)[0]
    # a valid call
    rc, msg = call(ev, pods, ids=ids)
    assert rc == last, msg
    assert ids_gone(ev, pods)[0]
    assert call(ev, pods[:0])[0] == last
    # the Python entry point raises it
    if last != abi.OK:
        with pytest.raises(KoordEvalError) as e:
            ev.diagnose(pods, T0, node_sets=ids, bitmaps=True)
        assert e.value.code == abi.ERR_NO_DEVICE
        assert ids_gone(ev, pods)[0]
