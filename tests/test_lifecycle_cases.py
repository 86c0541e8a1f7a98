"""CPU checks of tests/lifecycle_battery.py: the transition lists cover every family behind every kind of transition, the oracle's
answer is self-consistent, and the seeded lists do not move."""
import numpy as np

import lifecycle_battery as LB
import oracle_lib as O


def test_every_family_behind_every_transition():
    cells = LB.coverage()
    for kind in LB.TRANSITION_KINDS:
        for fam in LB.FAMILIES:
            assert cells.get((kind, fam), 0) >= 1, (kind, fam)
    assert {k for k, _ in cells} == set(LB.TRANSITION_KINDS)
    # each rps stop is reached at every rps shape under both windows, each reinit kind under both settings
    for rps in (1, 4096, 5, 0):
        assert cells[(f"rps {rps}", "wm_detect_keys")] == 2 * len(LB.RPS_SHAPES)
    for kind, shapes, how in LB.REINIT_CASES:
        assert cells[(kind, "wm_embed16")] == 2 * (len(shapes) - 1)
    shapes = {c[1] for c in LB.transition_cases()}
    assert shapes == {LB.S_SEQ, LB.S_STRIP, LB.S_SPLIT, LB.S_TILES, LB.S_TINY}
    assert {c[3]["max_frames"] for c in LB.transition_cases()} >= {1, 3}


def test_names_and_families_agree_with_the_oracle_dict():
    want3, want7 = LB.expectations(LB.S_TINY, p=3, F=2), LB.expectations(LB.S_TINY, p=7, F=1)
    assert {LB.family_of(n) for n in want3} == set(LB.FAMILIES) == {LB.family_of(n) for n in LB.names_of(3)}
    assert {LB.family_of(n) for n in want7} == set(LB.FAMILIES) == {LB.family_of(n) for n in LB.names_of(7)}
    assert not [n for n in want7 if "/ME" in n] and [n for n in want3 if "/ME" in n]
    heads = {n.rsplit(".", 1)[0] for n in want3}
    assert set(LB.names_of(3)) <= heads
    for kind, _ in want3.values():
        assert kind in LB.TOLERANCES


def test_expectations_are_self_consistent():
    shape, F = LB.S_SEQ, 3
    want = LB.expectations(shape, p=3, F=F)
    again = LB.expectations(shape, p=3, F=F)
    assert not LB.same_bits({n: v for n, (k, v) in want.items()}, {n: v for n, (k, v) in again.items()})
    as_dict = {n: v for n, (k, v) in want.items()}
    assert LB.check(as_dict, want) == []
    I, T = LB.inputs(shape), LB.tables(shape, F)
    for m in ("ME", "NVF"):
        # a batch is its frames: frame 0 of the queued embed is the one-frame embed
        assert np.array_equal(want[f"embed/{m}/f32/grey/Fq.y"][1][0], want[f"embed/{m}/f32/grey/F1.y"][1])
        assert want[f"embed/{m}/f32/grey/Fq.a"][1][0] == want[f"embed/{m}/f32/grey/F1.a"][1][0]
        # an all-plus table is the plain embed; the signs' strength is the embed's
        assert np.array_equal(want[f"embed_signs/{m}.a"][1], want[f"embed/{m}/f32/grey/Fq.a"][1])
        plus, zero = T["signs"] > 0, T["signs"] == 0
        assert plus.any() and zero.any() and (T["signs"] < 0).any()
        # the tile sums add up to the frame's score, and the detector of an embed's output sees the mark of W
        s = want[f"detect_tiles/{m}/f32.sums"][1]
        tot = s.sum(axis=(1, 2))
        assert np.abs(LB.TM.score_of(tot) - want[f"detect/{m}/f32/Fq.corr"][1]).max() <= LB.TOLERANCES["score"][0]
        assert (want[f"slot_out/{m}.corr"][1] > 0.1).all() and (want[f"detect/{m}/f32/Fq.corr"][1] > 0.1).all()
        # key banks: other keys do not answer, and the schedule picks the bank's column
        assert (np.abs(want[f"detect_keys/{m}/f32.corr"][1]) < 0.1).all()
        # the soft values decode nothing here (the frames carry W, not a payload), but a bit's score is bounded
        assert (np.abs(want[f"detect_bits/{m}.soft"][1]) <= 1).all()
    # the checker does see an error just beyond each bound
    bad = dict(as_dict)
    bad["embed/ME/f32/grey/F1.a"] = as_dict["embed/ME/f32/grey/F1.a"] * np.float32(1 + 3e-4)
    bad["detect/NVF/f32/F1.corr"] = as_dict["detect/NVF/f32/F1.corr"] + np.float32(3e-5)
    bad["pack16.v"] = as_dict["pack16.v"] ^ np.uint16(1)
    y = as_dict["embed/ME/u8/grey/F1.y"].copy()
    y.reshape(-1)[:40] ^= 1
    bad["embed/ME/u8/grey/F1.y"] = y
    assert [n for n, _ in LB.check(bad, want)] == sorted(["embed/ME/f32/grey/F1.a", "detect/NVF/f32/F1.corr", "pack16.v", "embed/ME/u8/grey/F1.y"])
    assert LB.same_bits(bad, as_dict) == sorted(["embed/ME/f32/grey/F1.a", "detect/NVF/f32/F1.corr", "pack16.v", "embed/ME/u8/grey/F1.y"])
    assert O.embed(I["xf32"][0], I["xf32"][0], I["W"])[0] == 0


def test_case_lists_are_stable_under_their_seed():
    a, b = LB.transition_cases(), LB.transition_cases()
    assert a == b and len(a) == len({repr(c) for c in a})
    # another seed deals another order of the rps legs; the set of cases is the same
    assert sorted(map(repr, LB.transition_cases(seed=1))) == sorted(map(repr, a))
    t1, t2 = LB.tables(LB.S_TILES, 3), LB.tables(LB.S_TILES, 3)
    for n in t1:
        assert np.array_equal(t1[n], t2[n]), n
    # pinned: the first entries the seed 4242 deals, and the layout of 2 x 16 tiles
    assert t1["signs"].shape == (3, 2, 16) and t1["multi"].shape == (3, LB.NCOPIES, 2, 16)
    assert t1["tile_bit"][3] == -1 and set(t1["tile_bit"]) == {-1, 0, 1, 2, 3, 4}
    assert np.array_equal(t1["tile_bit"], LB.BM.layout(2, 16, 5, 99) * (np.arange(32) != 3) - (np.arange(32) == 3))
    assert np.array_equal(t1["schedule"], LB.SM.schedule_walk(LB.K, LB.SCHEDULE_SEED, 0, 3))
    tiny = LB.tables(LB.S_TINY, 1)
    assert tiny["nbits"] == 1 and list(tiny["tile_bit"]) == [0]
