"""Every legal combination of a call's per-pod attachments on the device (attachments.py: sets x scores x domains x
{none, group ids, term lists} on 48 pods of spread_terms' input X in batches of 16): ke_eval of the first pods, then
ke_schedule, against the lock-step reference, and the count tables afterwards on the host and on the device.
test_attachments_host.py shows on the oracle that every kind present in a combination moves placements.  Every
comparison is exact."""
import numpy as np
import pytest

import attachments as A
from koordinator_amd import Evaluator, synth
from spread_terms import load, slice_kw

pytestmark = pytest.mark.gpu
T0 = synth.T0


@pytest.mark.parametrize("combo", A.COMBOS, ids=A.combo_id)
def test_eval_and_schedule_of_every_combination(gpu, combo):
    r = A.reference(combo)
    c, pods, kw = r["c"], r["pods"], r["kw"]
    ev = Evaluator(synth.config(c["n"], pod_batch=A.BATCH))
    synth.load_into(ev, c["cl"])
    load(ev, c)  # (every table, whatever the combination passes ids for)
    best, total = A.eval_reference(combo)
    got = ev.eval(pods[:A.N_EVAL], T0, **slice_kw(kw, 0, A.N_EVAL))
    assert np.array_equal(got["total"], total), np.argwhere(got["total"] != total)[:5].tolist()
    assert np.array_equal(got["best"], best)
    chosen, score = ev.schedule(pods, T0, **kw)
    assert np.array_equal(chosen, r["want"][0]), np.argwhere(chosen != r["want"][0])[:5].ravel().tolist()
    assert np.array_equal(score, r["want"][1]), np.argwhere(score != r["want"][1])[:5].ravel().tolist()
    for g in range(c["G"]):
        assert np.array_equal(ev.spread_groups_get(g + 1, c["n"]), r["counts_after"][g]), g + 1
    for g in range(len(r["dcounts_after"])):
        assert np.array_equal(ev.spread_domains_get(g + 1), r["dcounts_after"][g]), g + 1
    assert ev.debug_spread_groups_check() == 0
    assert ev.debug_spread_domains_check() == 0
