"""The references of test_gpu_attachments.py (attachments.py) on the oracle alone: in every combination of per-pod
attachments each kind present decides placements, so a device path that drops one cannot pass."""
import numpy as np
import pytest

import attachments as A


@pytest.mark.parametrize("combo", A.COMBOS, ids=A.combo_id)
def test_every_present_kind_moves_a_placement(combo):
    r = A.reference(combo)
    chosen, score = r["want"]
    assert len(chosen) == A.P and (chosen >= 0).all() and (score >= 0).all()
    for kind in range(4):
        if combo[kind]:
            moved = int((A.reference(A.without(combo, kind))["want"][0] != chosen).sum())
            assert moved >= 1, (A.combo_id(combo), kind)
    # the kinds that move counts do, the others leave the seeds
    c = r["c"]
    assert (r["counts_after"] != c["counts"]).any() == (combo[3] != 0)
    assert (r["dcounts_after"] != c["dom"]["dcounts"]).any() == bool(combo[2])


def test_the_slice_spans_three_batches_and_the_eval_reference_filters():
    assert A.P >= 3 * A.BATCH
    best, total = A.eval_reference((1, 1, 1, 2))
    plain_best, plain_total = A.eval_reference((0, 0, 0, 0))
    assert (best >= 0).all() and (plain_best >= 0).all()
    assert ((total == -1) & (plain_total >= 0)).any() and (total.max(1) > plain_total.max(1)).any()
