"""csrc/k_loop_candidates.h itself, compiled for the host (tests/cpp/lc_host_emu, -ffp-contract=off), against tests/ref_loop_candidates.py
over every case of loop_candidates_cases.py, exactly.  The checks, the bookkeeping, the row layout, the accumulation order, the tree, the
per-wave selection and its combination are checked here without a device.  Not a replacement for tests/test_gpu_loop_candidates.py: the
compiler, the wave butterfly, the barriers, LDS and the launches are not in it."""
import numpy as np
import pytest

import loop_candidates_cases as lc
import ref_loop_candidates as rl


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    return lc.EmuDriver(lc.emu_build(lc.ROOT, tmp_path_factory.mktemp("lc_host_emu")))


@pytest.mark.parametrize("name", list(lc.CASES))
def test_kernel_source_on_the_host_against_the_reference(drv, name):
    print(name, lc.check(name, drv))


def _cands(name):
    return [e for e in lc.reference(name) if e[0] == "candidates"]


def test_cases_reach_what_they_are_for():
    st = lambda e: [r[0] for r in e[3]]
    g = _cands("gap_by_id")                 # gaps 0, 19, 20, 21, 22; first the query at id 80 / 81, then the one at 79
    assert [e[3][0][3] for e in g[0::2]][:3] == [80, 80, 80] and [e[3][0][5] for e in g[0::2]] == [6, 5, 4, 3, 2]
    assert [e[3][0][3] for e in g[1::2]][:4] == [79, 79, 79, 79] and g[7][3][0][0] == rl.FOUND and g[9][3][0][0] != rl.FOUND
    # ids 80 and 81 hold one direction: the same bits, and the lower id is the answer while both are compared
    assert g[0][3][0][0] == rl.FOUND
    for name, want in (("tie_one_wave", 7), ("tie_two_waves", 9), ("tie_lower_id_in_a_later_wave", 15), ("tie_three_groups", 23)):
        (e,) = _cands(name)
        assert e[3][0][:2] == (rl.FOUND, want) and e[3][0][4] >= 2, name
    assert [st(e) for e in _cands("all_nonpositive")] == [[rl.NONE], [rl.NONE]]
    assert _cands("all_nonpositive")[0][3][0][4:] == (3, 5)                   # the rows at exactly 0 pass weak = -0.5 and are no best
    assert [st(e) for e in _cands("strong_at_own_bits")] == [[rl.FOUND], [rl.BELOW_STRONG], [rl.FOUND]]
    w = _cands("weak_at_own_bits")          # weak at the third-best row's bits, just below, just above; max_num_weak 1, 2, 3
    assert [e[3][0][4] for e in w] == [2, 2, 2, 3, 3, 3, 2, 2, 2]
    assert [st(e)[0] for e in w[:6]] == [rl.TOO_MANY_WEAK, rl.FOUND, rl.FOUND, rl.TOO_MANY_WEAK, rl.TOO_MANY_WEAK, rl.FOUND]
    assert [st(e) for e in _cands("n_weak_at_max")] == [[rl.TOO_MANY_WEAK], [rl.FOUND], [rl.FOUND]]
    b = _cands("bad_vectors")
    assert all(st(e) == [rl.FOUND, rl.BAD_VECTOR] for e in b[0::2]) and all(st(e) == [rl.BAD_VECTOR] for e in b[1::2])
    assert [e[2] for e in lc.reference("bad_vectors") if e[0] == "append"] == [True] + [False] * 5 + [True]
    five = _cands("five_streams")
    assert five[0] == five[1] and st(five[0])[0] == rl.NONE and rl.FOUND in st(five[0])
    assert [e[3][0] for e in five[2:7]] == five[0][3] and five[7][3] == [five[0][3][1], five[0][3][4]] and five[8][3] == []
    assert [e[2] for e in lc.reference("full_stream") if e[0] == "append"] == [True, False, False, True, False, True]
    ref = lc.reference("refusals")
    assert [e[2] for e in ref if e[0] == "configure"] == [False] * 6 + [True] * 3
    assert [e[2] for e in ref if e[0] == "append"] == [False, True] + [False] * 6
    assert [e[2] for e in ref if e[0] == "candidates"] == [False, False, True, False, True, False, False, False, False, True,
                                                           False, True, False, True] + [False] * 6 + [True]
    for n in (63, 64, 65):
        assert _cands("rows_%d" % n)[1][3][0][4:] == (n, n)
    big = _cands("rows_600_dim_4096")
    assert big[0][3][0][:2] == (rl.FOUND, 3 * 400 + 1) and big[1][3][0][5] == 600 and big[2][3][0][5] == 594


def test_read_returns_the_reference_rows_in_the_vector_order(drv):
    drv.configure(1, 2, 257)
    v = lc.vecs(4, 2, 257)
    assert drv.append([0, 0], [3, 8], v) is None
    ids, rows = drv.read(0)
    assert ids.tolist() == [3, 8] and np.array_equal(rows[0], rl.normalise(v[0])) and np.array_equal(rows[1], rl.normalise(v[1]))
