"""CPU checks of tests/sequence_model.py: the generator is deterministic and keeps slots from racing, the model's annotations
follow from the steps alone, and the committed seed list covers what tests/test_gpu_sequences.py is there to exercise -- every call
on an asynchronous slot, and every slot-state transition wm.h describes.  The counts are conditions on the seed list, not
measurements: a change of the generator that loses one must change the list."""
import collections

import pytest

import sequence_model as M


@pytest.fixture(scope="module")
def sequences():
    return [M.generate(seed) for seed in M.SEEDS]


def test_the_generator_is_deterministic(sequences):
    for seq in sequences[:8]:
        again = M.generate(seq.seed)
        assert again.steps == seq.steps and again.annotations == seq.annotations
        assert (again.handover, again.checked, again.fused) == (seq.handover, seq.checked, seq.fused)
    assert M.generate(1).steps != M.generate(2).steps
    assert len([s for s in M.generate(5, 6).steps if not s.get("auto")]) == 6


def test_the_model_alone_reproduces_the_annotations(sequences):
    for seq in sequences:
        anns, m = M.replay(seq)
        assert anns == seq.annotations
        assert m.gram == seq.model.gram and (m.trusted, m.redone) == (seq.model.trusted, seq.model.redone)


def test_sequences_are_valid_calls(sequences):
    for seq in sequences:
        assert len([s for s in seq.steps if not s.get("auto")]) == M.N_OPS
        for t in range(M.NSLOTS):
            assert not seq.model.slots[t]["reads"] and not seq.model.slots[t]["writes"], "a slot is left un-synced"
        for st in seq.steps:
            if st["kind"] == "caller_write":
                assert not seq.handover
            elif st["kind"] != "sync":
                assert 1 <= st["F"] <= M.MAX_F and st["slot"] in (0, 1, 2, M.SLOT_SYNC)


def test_a_race_between_slots_is_refused():
    m = M.Model(False, True, False)
    m.apply(dict(kind="embed", slot=0, mask=M.ME, F=2, variant="base_is_in", out=0, x0=0, b0=0))
    with pytest.raises(M.ModelError):
        m.apply(dict(kind="embed", slot=1, mask=M.ME, F=2, variant="base_is_in", out=0, x0=0, b0=0))
    with pytest.raises(M.ModelError):
        m.apply(dict(kind="detect", slot=1, mask=M.ME, F=1, src=("pool", 1, 1)))
    m.apply(dict(kind="sync", slot=0))
    m.apply(dict(kind="detect", slot=1, mask=M.ME, F=1, src=("pool", 1, 1)))


def test_the_model_states_wm_h():
    """the rules one by one, on hand-written steps"""
    emb = dict(kind="embed", slot=0, mask=M.ME, F=2, variant="base_is_in", out=0, x0=0, b0=0)
    det = dict(kind="detect", slot=0, mask=M.ME, F=2, src=("pool", 0, 2))
    # checked: trusted once, then used up; a caller's write makes that frame a redo
    m = M.Model(False, True, False)
    m.apply(emb)
    assert m.apply(det)["path"] == "checked" and m.apply(det)["path"] == "ordinary"
    m.apply(emb)
    m.apply(dict(kind="sync", slot=0))
    m.apply(dict(kind="caller_write", slot=None, frame=1, row=3, col=4))
    assert m.apply(det)["frame_paths"] == ["trusted", "redone"] and (m.trusted, m.redone) == (3, 1)
    assert m.gram == {"k_gram": 3, "k_gram_ho_checked": 2, "k_gram_redo": 2}
    # promised: only through WM_MEM_SLOT_OUT, and again for a second detector; a pointer takes the checked one
    m = M.Model(True, True, False)
    m.apply(emb)
    so = dict(kind="detect_keys", slot=0, mask=M.NVF, F=2, src=("slot_out",))
    assert m.apply(det)["path"] == "checked" and m.apply(det)["path"] == "ordinary"
    assert m.apply(so)["path"] == "promised" and m.apply(so)["path"] == "promised"
    assert m.apply(dict(det, src=("slot_out",)))["path"] == "promised"
    # wm_embed_signs: names the output, carries nothing; wm_embed_keys: changes nothing but ends what it overwrites
    m.apply(dict(emb, kind="embed_signs"))
    assert m.apply(so)["path"] == "ordinary" and m.slots[0]["last_by"] == "embed_signs"
    m.apply(emb)
    m.apply(dict(kind="embed_keys", slot=0, mask=M.ME, F=1, src=("fresh", 0), b0=0, out=3))
    assert m.slots[0]["ho"] is not None and m.slots[0]["last_out"] == (0, 2)
    m.apply(dict(kind="embed_keys", slot=0, mask=M.ME, F=1, src=("fresh", 0), b0=0, out=0))
    assert m.slots[0]["ho"] is None and m.slots[0]["last_out"] == (0, 2)
    # the pair hands over by itself, and without wm_set_handover nothing of that outlives it
    m = M.Model(False, False, False)
    assert m.apply(dict(emb, kind="embed_detect"))["path"] == "promised"
    assert m.apply(dict(det, src=("slot_out",)))["path"] == "ordinary"
    # one frame, a base that is the output: no hand-over; in place: one (the stencil reads the snapshot)
    m = M.Model(True, True, True)
    for variant, F, held in (("base_is_in", 1, False), ("base_is_out", 2, False), ("in_place", 2, True)):
        m.apply(dict(emb, variant=variant, F=F))
        assert (m.slots[0]["ho"] is not None) == held
    # a synchronous one-frame call takes the fused kernels and no hand-over
    m.apply(emb)
    assert m.apply(dict(kind="detect", slot=M.SLOT_SYNC, mask=M.ME, F=1, src=("pool", 0, 1)))["path"] == "fused"
    assert m.apply(dict(emb, slot=M.SLOT_SYNC, F=1))["path"] == "fused" and m.slots[0]["ho"] is None


def test_every_call_runs_on_an_asynchronous_slot(sequences):
    seen = collections.Counter(st["kind"] for seq in sequences for st in seq.steps if st["kind"] != "caller_write" and st["slot"] != M.SLOT_SYNC)
    for kind in M.KINDS:
        assert seen[kind] >= 10, (kind, seen[kind])
    sync_calls = collections.Counter(st["kind"] for seq in sequences for st in seq.steps if st.get("slot") == M.SLOT_SYNC)
    assert sum(sync_calls.values()) >= 20, sync_calls
    assert sum(1 for seq in sequences for a in seq.annotations if a["path"] == "fused") >= 4


def test_the_oracle_anchors_are_there(sequences):
    """tests/test_gpu_sequences.py holds the first wm_embed and the first wm_detect of a sequence to the CPU oracle, whatever plane
    they read; nearly every sequence has both, and each has one"""
    with_embed = sum(any(st["kind"] == "embed" for st in seq.steps) for seq in sequences)
    with_detect = sum(any(st["kind"] == "detect" for st in seq.steps) for seq in sequences)
    assert with_embed >= 44 and with_detect >= 38, (with_embed, with_detect)
    assert all(any(st["kind"] in ("embed", "detect") for st in seq.steps) for seq in sequences)
    sources = collections.Counter(next(st["src"][0] for st in seq.steps if st["kind"] == "detect")
                                  for seq in sequences if any(st["kind"] == "detect" for st in seq.steps))
    assert min(sources[k] for k in ("fresh", "pool", "slot_out")) >= 5, sources


def test_every_transition_occurs(sequences):
    total = collections.Counter()
    for seq in sequences:
        total.update(seq.model.transitions)
    for name in M.TRANSITIONS:
        assert total[name] >= 2, (name, dict(total))
    # a promised hand-over is taken through WM_MEM_SLOT_OUT by wm_detect and by at least two other detector kinds
    others = [k for k in M.DETECTORS if k != "detect" and total["promised_taken:" + k] >= 2]
    assert len(others) >= 2, dict(total)
    assert sum(seq.model.redone for seq in sequences) >= 2 and sum(seq.model.trusted for seq in sequences) >= 4
    assert {(s.handover, s.checked) for s in sequences} == {(False, False), (False, True), (True, False), (True, True)}
