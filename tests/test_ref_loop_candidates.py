"""tests/ref_loop_candidates.py held to facts that do not come from it: its two forms of every function agree; a scalar loop written here
gives the same bits; the butterfly's lane 0 is the halving tree; the f32 similarity lies within a derived bound of the f64 dot product;
the tie rule and the strictness of each compare.  CPU only."""
import numpy as np
import pytest

import ref_loop_candidates as rl

f32 = np.float32
U = 2.0 ** -24                       # unit roundoff of f32, round to nearest
DIMS = (1, 2, 63, 64, 65, 128, 200, 1280, 4096)


def gamma(n):
    return n * U / (1 - n * U)


def scalar_similarity(a, b):
    """the contract once more, one f32 operation per line"""
    acc = [f32(0)] * 64
    for e in range(len(a)):
        p = f32(f32(a[e]) * f32(b[e]))
        acc[e % 64] = f32(acc[e % 64] + p)
    for s in (32, 16, 8, 4, 2, 1):
        for l in range(s):
            acc[l] = f32(acc[l] + acc[l + s])
    return acc[0]


@pytest.mark.parametrize("dim", DIMS)
def test_similarity_forms_agree(dim):
    rng = np.random.default_rng(dim)
    rows = rng.standard_normal((5, dim)).astype(f32); q = rng.standard_normal(dim).astype(f32)
    batch = rl.similarity_rows(q, rows)
    for r, s in zip(rows, batch):
        one = rl.similarity(q, r)
        assert one.dtype == f32 and one.view(np.uint32) == s.view(np.uint32) == scalar_similarity(q, r).view(np.uint32)


def test_butterfly_lane_0_is_the_tree_and_all_lanes_agree():
    rng = np.random.default_rng(1)
    for _ in range(200):
        acc = (rng.standard_normal(64) * 10.0 ** rng.integers(-6, 6, 64)).astype(f32)
        b = rl.butterfly(acc)
        assert b[0].view(np.uint32) == rl.tree(acc).view(np.uint32)
        assert np.all(b.view(np.uint32) == b[0].view(np.uint32))


@pytest.mark.parametrize("dim", DIMS)
def test_similarity_within_the_derived_bound_of_f64(dim):
    """A term a[e] b[e] reaches acc[0] through 1 rounded product, at most ceil(dim / 64) rounded sums inside its accumulator and 6 in the
    tree: n = ceil(dim / 64) + 7 roundings, each (1 + d), |d| <= u.  So |sim - sum a b| <= gamma_n sum |a b|, gamma_n = n u / (1 - n u)
    (Higham, Accuracy and Stability, lemma 3.1), plus 2^-149 per product that might round in the subnormal range.

    The normalisation: n2 is a sum of positive terms by the same chain, so n2 = |a|^2 (1 + t), |t| <= gamma_n; the square root halves
    that and rounds once, the division rounds once: v[e] = a[e] / |a| (1 + h), |h| <= eta = gamma_n / 2 + 2 u + (second order, covered
    by taking gamma_n whole).  Against the cosine of the raw vectors each term of the sum is then off by (1 + eta)^2 - 1, and the
    rounding bound applies to the terms as they are: |sim - cos| <= (gamma_n (1 + eta)^2 + (1 + eta)^2 - 1) sum |a b| / (|a| |b|)."""
    rng = np.random.default_rng(100 + dim)
    n = -(-dim // 64) + 7
    eta = gamma(n) + 2 * U
    for trial in range(20):
        a = rng.standard_normal(dim).astype(f32); b = (a + rng.standard_normal(dim) * 10.0 ** -(trial % 4)).astype(f32)
        s = float(rl.similarity(a, b))
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        assert abs(s - a64 @ b64) <= gamma(n) * np.sum(np.abs(a64 * b64)) + dim * 2.0 ** -149
        na, nb = rl.normalise(a), rl.normalise(b)
        cos = a64 @ b64 / np.sqrt((a64 @ a64) * (b64 @ b64))
        mag = np.sum(np.abs(a64 * b64)) / np.sqrt((a64 @ a64) * (b64 @ b64))
        assert abs(float(rl.similarity(na, nb)) - cos) <= (gamma(n) * (1 + eta) ** 2 + (1 + eta) ** 2 - 1) * mag + dim * 2.0 ** -149
        assert abs(float(rl.similarity(na, na)) - 1) <= (gamma(n) * (1 + eta) ** 2 + (1 + eta) ** 2 - 1) + dim * 2.0 ** -149


def test_normalise_refuses_what_has_no_direction():
    assert rl.normalise(np.zeros(7, f32)) is None
    assert rl.normalise(np.array([1, np.inf], f32)) is None and rl.normalise(np.array([np.nan, 1], f32)) is None
    assert rl.normalise(np.full(65, 3e19, f32)) is None and rl.normalise(np.full(65, 1e-30, f32)) is None
    v = rl.normalise(np.array([3, 4], f32))
    assert v.dtype == f32 and np.array_equal(v, np.array([3, 4], f32) / f32(5))


def test_selection_forms_agree():
    rng = np.random.default_rng(5)
    levels = np.array([-0.5, 0.0, 0.2, 0.93, 0.94, 0.95, 0.97], f32)
    seen = set()
    for _ in range(3000):
        n = int(rng.integers(0, 9))
        ids = np.sort(rng.choice(60, n, replace=False))
        sims = levels[rng.integers(0, len(levels), n)]
        args = (int(rng.integers(40, 70)), ids, sims, 0.93, 0.95, int(rng.integers(0, 4)), int(rng.integers(0, 30)))
        a, b = rl.select(*args), rl.select_vec(*args)
        assert a == b, (args, a, b)
        seen.add(a[0])
    assert seen == {rl.FOUND, rl.NONE, rl.BELOW_STRONG, rl.TOO_MANY_WEAK}


def test_tie_rule_and_strict_compares():
    sel = lambda ids, sims, kf=100, weak=0.93, strong=0.95, m=3, gap=20: rl.select(kf, ids, np.array(sims, f32), weak, strong, m, gap)
    hi = f32(0.97)
    assert sel([3, 5, 9], [hi, hi, hi])[1] == 3                                     # the lowest id wins a tie
    assert sel([3, 5], [0.0, 0.0])[0] == rl.NONE and sel([3], [-0.2])[0] == rl.NONE     # sim > 0, strictly
    assert sel([3], [np.nextafter(f32(0), f32(1))], strong=0.0)[0] == rl.FOUND
    s = f32(0.95)
    assert sel([3], [s], strong=s)[0] == rl.FOUND                                   # best < strong, strictly
    assert sel([3], [s], strong=np.nextafter(s, f32(1)))[0] == rl.BELOW_STRONG
    w = f32(0.96)
    assert sel([1, 2, 3, 4], [hi, w, w, w], weak=w)[4] == 1                         # sim > weak, strictly, and the best is counted
    assert sel([1, 2, 3, 4], [hi, w, w, w], weak=np.nextafter(w, f32(0)))[4] == 4
    assert sel([1, 2, 3, 4], [hi, w, w, w], weak=0.9, m=4)[0] == rl.FOUND           # n_weak > max_num_weak, strictly
    assert sel([1, 2, 3, 4], [hi, w, w, w], weak=0.9, m=3)[0] == rl.TOO_MANY_WEAK
    assert sel([79, 80, 81], [w, hi, hi])[3] == 80 and sel([79, 80, 81], [w, hi, hi])[5] == 2      # kf_id - id < min_gap, by id
    assert sel([79, 80, 81], [w, w, hi], gap=19)[3] == 81
    assert sel([1], [0.5])[:2] == (rl.BELOW_STRONG, -1) and sel([1], [0.5])[3] == 1     # best_kf is reported without a candidate
    assert sel([], []) == (rl.NONE, -1, f32(0), -1, 0, 0)
    # the order of the outcomes: below strong is said before too many weak
    assert sel([1, 2, 3, 4, 5], [0.94] * 5, weak=0.5, m=1)[0] == rl.BELOW_STRONG


def test_store_bookkeeping():
    S = rl.Store()
    assert S.append([0], [0], np.ones((1, 4))) == "the store is not configured"
    assert S.configure(1, 2, 0) and S.configure(1, 2, 4097) and S.configure(2, 2, 4) is None
    assert S.append([0, 0], [4, 4], np.ones((2, 4))) and S.count(0) == 0
    assert S.append([0, 1], [4, 0], np.ones((2, 4))) is None and S.append([0], [4], np.ones((1, 4)))
    assert S.append([0, 0], [5, 6], np.ones((2, 4))) == "the stream is full" and S.count(0) == 1
    assert S.append([0], [5], np.zeros((1, 4))).startswith("a vector cannot be normalised")
    ids, rows = S.read(0)
    assert ids.tolist() == [4] and np.array_equal(rows, np.full((1, 4), 0.5, f32))
    assert isinstance(S.candidates([(0, 4)], np.ones((1, 4))), str) and isinstance(S.candidates([(1, 9), (0, 9)], np.ones((2, 4))), str)
    r = S.candidates([(0, 24)], np.ones((1, 4)), strong=1.0)
    assert r == [(rl.FOUND, 4, f32(1), 4, 1, 1)]
    assert S.candidates([(0, 24)], np.zeros((1, 4)))[0][0] == rl.BAD_VECTOR
