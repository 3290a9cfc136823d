"""The loop candidate search, written from the reference's src/loopclosure.cpp:173-284 (SimilarityScore, AddNewKeyFrame,
LoopKeyframeCandidate) and :128 (the normalisation), in numpy, f32 step by step.  This is the contract that csrc/k_loop_candidates.h, its
host build and this module meet bit for bit (include/svslam.h states it; DESIGN 13 lists the deviations from the reference):

  similarity   64 accumulators from +0; accumulator l takes the elements l, l + 64, ... below dim in that order,
               acc = acc + (a[e] * b[e]), product and sum each rounded to f32; then acc[l] += acc[l + s] for l < s, s = 32 .. 1; acc[0].
  normalise    n2 = similarity(a, a); a[e] / sqrt(n2); n2 zero or not finite: BAD_VECTOR (None here).
  select       rows in ascending id; kf_id - id < min_gap skipped; best = the largest sim > 0, the lowest id on a tie; n_weak counts
               sim > weak; NONE, then best < strong, then n_weak > max_num_weak, then FOUND.

Two forms of most functions stand side by side (a per-row loop and a vectorised one); tests/test_ref_loop_candidates.py holds them to
each other and to facts that do not come from this file."""
import numpy as np

FOUND, NONE, BELOW_STRONG, TOO_MANY_WEAK, BAD_VECTOR = 0, 1, 2, 3, 4
STATUS_NAMES = ["FOUND", "NONE", "BELOW_STRONG", "TOO_MANY_WEAK", "BAD_VECTOR"]
MAX_DIM = 4096
DEFAULTS = dict(weak=0.93, strong=0.95, max_num_weak=3, min_gap=20)     # tests/golden/config-00.yaml; the gap is :244's literal

f32 = np.float32


def accumulators(a, b):
    """the 64 accumulators before the tree"""
    a = np.asarray(a, f32); b = np.asarray(b, f32)
    assert a.ndim == 1 and a.shape == b.shape
    with np.errstate(all="ignore"):
        prod = a * b                                        # f32 products, each rounded
        acc = np.zeros(64, f32)
        for k in range(0, len(a), 64):
            m = min(64, len(a) - k)
            acc[:m] = acc[:m] + prod[k:k + m]
    return acc


def tree(acc):
    acc = np.array(acc, f32)
    with np.errstate(all="ignore"):
        for s in (32, 16, 8, 4, 2, 1):
            acc[:s] = acc[:s] + acc[s:2 * s]
    return acc[0]


def butterfly(acc):
    """what a wave does without LDS: every lane adds its partner's value; all 64 lanes of the result"""
    acc = np.array(acc, f32)
    lanes = np.arange(64)
    with np.errstate(all="ignore"):
        for s in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[lanes ^ s]
    return acc


def similarity(a, b):
    return tree(accumulators(a, b))


def similarity_rows(q, rows):
    """similarity of q with every row of rows [n, dim], vectorised over the rows"""
    q = np.asarray(q, f32); rows = np.asarray(rows, f32).reshape(-1, len(q))
    with np.errstate(all="ignore"):
        prod = rows * q[None, :]
        acc = np.zeros((len(rows), 64), f32)
        for k in range(0, len(q), 64):
            m = min(64, len(q) - k)
            acc[:, :m] = acc[:, :m] + prod[:, k:k + m]
        for s in (32, 16, 8, 4, 2, 1):
            acc[:, :s] = acc[:, :s] + acc[:, s:2 * s]
    return acc[:, 0].copy()


def normalise(a):
    """a / |a| in f32, or None where the contract says BAD_VECTOR"""
    a = np.asarray(a, f32)
    n2 = similarity(a, a)
    if not (np.isfinite(n2) and n2 > 0):
        return None
    with np.errstate(all="ignore"):
        return a / np.sqrt(f32(n2))


def select(kf_id, ids, sims, weak, strong, max_num_weak, min_gap):
    """LoopKeyframeCandidate's loop, row by row -> (status, cand_kf, best_sim, best_kf, n_weak, n_compared)"""
    best, best_id, n_weak, n_cmp = f32(0), -1, 0, 0
    for i, s in zip(ids, sims):
        if kf_id - int(i) < min_gap:
            continue
        n_cmp += 1
        if s > best:
            best, best_id = f32(s), int(i)
        if s > f32(weak):
            n_weak += 1
    if best_id < 0:
        st = NONE
    elif best < f32(strong):
        st = BELOW_STRONG
    elif n_weak > max_num_weak:
        st = TOO_MANY_WEAK
    else:
        st = FOUND
    return (st, best_id if st == FOUND else -1, f32(best), best_id, n_weak, n_cmp)


def select_vec(kf_id, ids, sims, weak, strong, max_num_weak, min_gap):
    """the same by masks and argmax (np.argmax returns the first of equal maxima, and the ids ascend)"""
    ids = np.asarray(ids, np.int64); sims = np.asarray(sims, f32)
    keep = (kf_id - ids) >= min_gap
    ids, sims = ids[keep], sims[keep]
    n_weak = int(np.sum(sims > f32(weak)))
    pos = sims > 0
    if not pos.any():
        return (NONE, -1, f32(0), -1, n_weak, len(ids))
    k = int(np.argmax(np.where(pos, sims, f32(-np.inf))))
    best, best_id = sims[k], int(ids[k])
    st = BELOW_STRONG if best < f32(strong) else TOO_MANY_WEAK if n_weak > max_num_weak else FOUND
    return (st, best_id if st == FOUND else -1, f32(best), best_id, n_weak, len(ids))


class Store:
    """the resident store's second reading: the same calls, the same refusals (a refusal returns its reason and changes nothing)"""

    def __init__(self):
        self.nstreams = 0

    def configure(self, nstreams, capacity, dim):
        if nstreams < 1 or capacity < 1:
            return "nstreams and capacity must be at least 1"
        if not 1 <= dim <= MAX_DIM:
            return "dim must be 1 .. 4096"
        self.nstreams, self.capacity, self.dim = nstreams, capacity, dim
        self.ids = [[] for _ in range(nstreams)]
        self.rows = [[] for _ in range(nstreams)]
        return None

    def append(self, streams, kf_ids, vecs):
        if self.nstreams == 0:
            return "the store is not configured"
        vecs = np.asarray(vecs, f32).reshape(len(streams), self.dim)
        cnt = [len(i) for i in self.ids]; last = [i[-1] if i else -1 for i in self.ids]
        new = []
        for s, k, v in zip(streams, kf_ids, vecs):
            if not 0 <= s < self.nstreams:
                return "unknown stream"
            if k < 0:
                return "negative keyframe id"
            if cnt[s] >= self.capacity:
                return "the stream is full"
            if k <= last[s]:
                return "keyframe ids must ascend strictly within a stream"
            cnt[s] += 1; last[s] = k
            new.append((s, int(k), normalise(v)))
        for i, (_, _, n) in enumerate(new):
            if n is None:
                return "a vector cannot be normalised (BAD_VECTOR): row %d" % i
        for s, k, n in new:
            self.ids[s].append(k); self.rows[s].append(n)
        return None

    def candidates(self, jobs, vecs, weak=DEFAULTS["weak"], strong=DEFAULTS["strong"], max_num_weak=DEFAULTS["max_num_weak"],
                   min_gap=DEFAULTS["min_gap"]):
        """jobs: [(stream, kf_id)] -> reason, or the list of select()'s tuples"""
        if self.nstreams == 0:
            return "the store is not configured"
        if min_gap < 0:
            return "negative min_gap"
        if max_num_weak < 0:
            return "negative max_num_weak"
        if not (np.isfinite(f32(weak)) and np.isfinite(f32(strong))):
            return "a threshold is not finite"
        vecs = np.asarray(vecs, f32).reshape(len(jobs), self.dim)
        prev = None
        for s, k in jobs:
            if not 0 <= s < self.nstreams:
                return "unknown stream"
            if prev is not None and s <= prev:
                return "streams must ascend, one job per stream"
            if self.ids[s] and k <= self.ids[s][-1] or k < 0:
                return "kf_id must be above the stream's last stored id"
            prev = s
        out = []
        for (s, k), v in zip(jobs, vecs):
            q = normalise(v)
            if q is None:
                out.append((BAD_VECTOR, -1, f32(0), -1, 0, 0))
                continue
            sims = similarity_rows(q, np.array(self.rows[s], f32).reshape(-1, self.dim)) if self.ids[s] else np.zeros(0, f32)
            out.append(select(k, self.ids[s], sims, weak, strong, max_num_weak, min_gap))
        return out

    def count(self, stream):
        return len(self.ids[stream])

    def read(self, stream):
        return np.array(self.ids[stream], np.int32), np.array(self.rows[stream], f32).reshape(-1, self.dim)
