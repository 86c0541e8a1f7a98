"""CPU tests of wm_key_schedule against its numpy restatement (tests/select_model.py): the table for every seed, first frame and bank
size of the grid, the restatement against the generator walked from frame 0, the cut-anywhere property, and the argument errors (no
GPU needed)."""
import ctypes as C

import numpy as np
import pytest

import select_model as SM

SEEDS = (0, 1, 2 ** 64 - 1)
FIRSTS = (0, 7, 2 ** 40)
NKEYS = (1, 3, 4096)
FRAMES = 64


def lib_schedule(wm, nkeys, seed, first, frames):
    out = np.full(frames, -7, np.int32)
    rc = wm.lib().wm_key_schedule(nkeys, seed, first, frames, out.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == wm.WM_OK, rc
    return out


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("nkeys", NKEYS)
def test_library_equals_model(wm, seed, first, nkeys):
    got = lib_schedule(wm, nkeys, seed, first, FRAMES)
    want = SM.schedule(nkeys, seed, first, FRAMES)
    assert got.dtype == np.int32 and np.array_equal(got, want), (got, want)
    assert got.min() >= 0 and got.max() < nkeys
    assert np.array_equal(got, [SM.z_of(seed, first + i) % nkeys for i in range(FRAMES)])
    assert np.array_equal(wm.Watermark.key_schedule(nkeys, seed, first, FRAMES), want)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("first", (0, 7))
def test_model_is_the_documented_generator(seed, first):
    """the direct form is splitmix64 walked from the seed"""
    assert np.array_equal(SM.schedule(5, seed, first, 40), SM.schedule_walk(5, seed, first, 40))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("nkeys", NKEYS)
def test_a_clip_takes_its_schedule_from_its_first_frame(wm, seed, first, nkeys):
    whole = lib_schedule(wm, nkeys, seed, first, 24)
    for i in (0, 1, 5, 23):
        assert lib_schedule(wm, nkeys, seed, first + i, 1)[0] == whole[i], i
        assert np.array_equal(lib_schedule(wm, nkeys, seed, first + i, 24 - i), whole[i:])


def test_wraps_at_the_end_of_the_frame_counter(wm):
    """first_frame + i runs modulo 2^64 like the state itself"""
    got = lib_schedule(wm, 4096, 3, 2 ** 64 - 2, 4)
    assert np.array_equal(got, SM.schedule(4096, 3, 2 ** 64 - 2, 4))
    assert got[2] == SM.z_of(3, 0) % 4096


def test_a_schedule_uses_the_whole_bank(wm):
    got = lib_schedule(wm, 4, 99, 0, 256)
    assert sorted(set(got.tolist())) == [0, 1, 2, 3]
    assert np.bincount(got, minlength=4).min() >= 32  # (expected 64 each)


@pytest.mark.parametrize("mask", (0, 1))
def test_oracle_alone_separates_the_schedules(mask):
    """the round trip tests/test_gpu_select.py runs on the library, on the CPU oracle alone: with the frames, keys and seeds of
    select_model.round_trip_case the weakest score under the right schedule is more than 4 times the largest |score| under the
    schedule rotated by one key (the factor test_gpu_keys.py::test_identification asserts at this shape and strength), under ME and
    under NVF -- about 30 times in both"""
    xs, Ws, table, rotated = SM.round_trip_case()
    assert len(set(table.tolist())) >= 3 and np.all(table != rotated)
    ys, right, wrong = SM.oracle_round_trip(xs, Ws, table, rotated, mask=mask)
    print("right", right, "wrong", wrong)
    assert right.min() > 4 * np.abs(wrong).max(), (right, wrong)


def test_argument_errors(wm):
    L = wm.lib()
    out = np.full(4, -7, np.int32)
    p = out.ctypes.data_as(C.POINTER(C.c_int32))
    bad = wm.WM_ERR_BAD_ARG
    assert L.wm_key_schedule(0, 1, 0, 4, p) == bad
    assert L.wm_key_schedule(-1, 1, 0, 4, p) == bad
    assert L.wm_key_schedule(4097, 1, 0, 4, p) == bad
    assert L.wm_key_schedule(3, 1, 0, 0, p) == bad
    assert L.wm_key_schedule(3, 1, 0, -2, p) == bad
    assert L.wm_key_schedule(3, 1, 0, 4, None) == bad
    assert np.all(out == -7)  # (a refused call writes nothing)
    assert L.wm_key_schedule(4096, 1, 0, 4, p) == wm.WM_OK and L.wm_key_schedule(1, 1, 0, 1, p) == wm.WM_OK
    for args in ((0, 1, 0, 4), (3, 1, 0, 0)):
        with pytest.raises(RuntimeError):
            wm.Watermark.key_schedule(*args)
