"""CPU: the planner's decisions and the packed blobs against the snapshot recorded in tests/golden/plan_snapshot.json (tests/plan_snapshot.py
says what is recorded and how to regenerate it).  A refactor of the planner, the dispatcher or the packer must leave every digest as it is; a
change that moves a plan on purpose regenerates the file and says which handles moved."""
import json

import plan_snapshot as S


def _recorded():
    with open(S.PATH) as f:
        return json.load(f)


def test_every_plan_of_the_matrix_is_the_recorded_one():
    want = _recorded()["plans"]
    handles = dict(S.plan_handles())
    assert set(handles) == set(want), "the handle matrix and the recorded file disagree: %s" % sorted(set(handles) ^ set(want))[:5]
    moved = [k for k, kw in handles.items() if S.digest(S.plan_record(kw)) != want[k]]
    assert not moved, "%d plans moved (python tests/plan_snapshot.py --dump KEY prints one in full), e.g. %s" % (len(moved), moved[:5])


def test_every_packed_blob_is_the_recorded_one():
    want = _recorded()["blobs"]
    handles = dict(S.blob_handles())
    assert set(handles) == set(want)
    moved = [k for k, kw in handles.items() if S.blob_digest(kw) != want[k]]
    assert not moved, "%d blobs differ from the recorded ones: %s" % (len(moved), moved)
