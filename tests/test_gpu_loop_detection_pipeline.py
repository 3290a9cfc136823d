"""Pipeline.detect_loops (product library) on two synthetic streams for 30 frames, against a second reading of its bookkeeping written here
in plain Python over tests/ref_loop_candidates.py and tests/ref_loop_verify.py (the stored descriptors it verifies with are held to
tests/ref_brief.py by test_gpu_brief_pipeline.py).  min_gap = 2 and keyframes_to_ignore_after_loop = 1, so that 30 frames reach the
branches.  The global descriptors are planted: a deterministic vector per (stream, keyframe); on stream 0 every keyframe from the third on
is a noisy copy of the vector min_gap keyframes back, on stream 1 every third one is; one vector is zero (BAD_VECTOR).  After EVERY step
detect_loops must equal the second reading: skipped / searched / verified / stored, the candidate's outputs bit for bit, the store's ids,
the verification's outputs at DESIGN 11's tolerances, the last closed keyframe.  ACCEPTED is the references' decision, so the equality
is what is asserted.

Measured once, streams 51 / 52, 5 / 6 keyframes in 30 frames: at min_gap = 2 the references accept no pair, neither at the
configuration's min_matches = 20 nor at 10: keyframes two apart keep 35 / 18 / 67 matches on stream 0 of which 4 / 0-4 / 4 are RANSAC
inliers (FEW_INLIERS, FEW_MATCHES).  The accepted branch (last closed keyframe set, the keyframe not stored, the next keyframe skipped,
one more edge in a following pose-graph optimisation) is therefore reached by a third case, min_gap = 1 at min_matches = 10, where
the candidate is the keyframe before: the pair test_gpu_brief_pipeline.py reaches ACCEPTED with."""
import importlib

import numpy as np
import pytest

import loop_candidates_cases as lcc
import loop_verify_cases as lvc
import ref_loop_candidates as rc
import ref_loop_verify as rv

pytestmark = pytest.mark.gpu
NFRAMES = 30
SEEDS = (51, 52)
DIM = 1280
CAND_DEFAULT = dict(weak=0.93, strong=0.95, max_num_weak=3)
IGNORE = 1
_VEC = {}


def planted(gap, s, k):
    """the global descriptor of keyframe k of stream s.  gap 2: every keyframe of stream 0 from the third on copies the one two back.
    gap 1: the odd keyframes of stream 0 copy the one before, the even ones are fresh, so that the copies do not pile up as weak rows."""
    if (gap, s, k) not in _VEC:
        base = np.random.default_rng(1000 * s + k).standard_normal(DIM).astype(np.float32)
        copy0 = k >= 2 if gap == 2 else k % 2 == 1
        if s == 1 and k == 1:
            v = np.zeros(DIM, np.float32)                   # cannot be normalised
        elif (s == 0 and copy0) or (s == 1 and k >= 3 and k % 3 == 0):
            src = planted(gap, s, k - gap)
            v = lcc.near(src if src.any() else base, 7 * k + s, 0.01)
        else:
            v = base
        _VEC[(gap, s, k)] = v
    return _VEC[(gap, s, k)]


@pytest.mark.parametrize("min_gap,min_matches", ((2, 20), (2, 10), (1, 10)))
def test_detect_loops_equals_its_second_reading(svs, min_gap, min_matches):
    CAND = dict(CAND_DEFAULT, min_gap=min_gap)
    pl = importlib.import_module("stereovision-slam_amd.pipeline")
    p = pl.Pipeline(pl.default_config(device_map=0), nstreams=2)
    p.keep_keyframe_features(True)
    cam = np.array(p.cfg.cam_l); ext_l = np.array(p.cfg.ext_l)
    prm = dict(min_matches=min_matches, min_pose_difference=1.0, max_pose_difference=50.0, max_pose_distance=20.0)    # the config's values
    ref = rc.Store()
    nkf, last_closed, accepted, skipped, statuses = [0, 0], [-1, -1], [0, 0], [0, 0], set()
    vecs = np.zeros((2, DIM), np.float32)
    for i in range(NFRAMES):
        pairs = [svs.synth_pair(sd, i) for sd in SEEDS]
        r = p.step([a for a, _ in pairs], [b for _, b in pairs])
        new = [s for s in range(2) if r["is_keyframe"][s]]
        if i == 0:
            assert new == [0, 1]
            with pytest.raises(RuntimeError, match="not configured"):
                p.detect_loops(vecs, IGNORE, **CAND, **prm)
            p.loopdb_configure(64, DIM); assert ref.configure(2, 64, DIM) is None
            with pytest.raises(RuntimeError, match="never described"):
                p.detect_loops(vecs, IGNORE, **CAND, **prm)
        assert p.describe_new_keyframes() == len(new)
        for s in new:
            vecs[s] = planted(min_gap, s, nkf[s])
        # the second reading, as far as it needs no device: the skip rule and the candidates
        want = [dict(is_keyframe=s in new, skipped=False, searched=False, verified=False, stored=False, kf_id=nkf[s] if s in new else -1)
                for s in range(2)]
        jobs = []
        for s in new:
            if last_closed[s] >= 0 and nkf[s] - last_closed[s] <= IGNORE:
                want[s]["skipped"] = True; skipped[s] += 1
            else:
                jobs.append((s, nkf[s]))
        cands = ref.candidates(jobs, vecs[[s for s, _ in jobs]], **CAND) if jobs else []
        got = p.detect_loops(vecs, IGNORE, **CAND, **prm)
        assert all(not g["is_keyframe"] for g in p.detect_loops(vecs, IGNORE, **CAND, **prm))       # a keyframe is handled once
        # the verification's inputs are the map as detect_loops left it
        store = []
        for (s, k), c in zip(jobs, cands):
            want[s]["searched"] = True
            g = got[s]
            assert g["cand"] is not None, (i, s)
            assert (g["cand"]["status"], g["cand"]["cand_kf"], lcc.bits(g["cand"]["best_sim"]), g["cand"]["best_kf"], g["cand"]["n_weak"],
                    g["cand"]["n_compared"]) == lcc._result(c), (i, s, g["cand"], c)
            statuses.add(c[0])
            ok_loop = False
            if c[0] == rc.FOUND:
                want[s]["verified"] = True
                fq, fc = p.keyframe_features(s, k), p.keyframe_features(s, c[1])
                (dq, rq), (dc, rcand) = p.keyframe_descriptors(s, k), p.keyframe_descriptors(s, c[1])
                job = dict(desc_c=dc, desc_q=dq, xyz_c=fc["xyz"][rcand], has_xyz=fc["has_xyz"][rcand], uv_q=fq["xy"][rq], T_cur=fq["pose"],
                           T_cand=fc["pose"])
                lref = rv.loop_verify(job, cam, ext_l, **prm)
                assert g["loop"] is not None, (i, s)
                ok, msg = lvc.compare(g["loop"], lref)
                print("frame %d stream %d: keyframe %d against %d: %s, %d matches, %d inliers" % (i, s, k, c[1], rv.STATUS_NAMES[lref["status"]],
                                                                                               lref["n_matches"], lref["n_inliers"]))
                assert ok, (i, s, msg)
                ok_loop = lref["status"] == rv.ACCEPTED
            if ok_loop:
                last_closed[s] = k; accepted[s] += 1
            elif c[0] != rc.BAD_VECTOR:
                store.append((s, k)); want[s]["stored"] = True
        if store:
            assert ref.append([s for s, _ in store], [k for _, k in store], vecs[[s for s, _ in store]]) is None
        for s in range(2):
            g = got[s]
            assert {k: g[k] for k in want[s]} == want[s], (i, s, g, want[s])
            assert (g["cand"] is None) == (not want[s]["searched"]) and (g["loop"] is None) == (not want[s]["verified"])
            assert p.loopdb_ids(s).tolist() == ref.read(s)[0].tolist(), (i, s)
            assert p.last_closed_keyframe(s) == last_closed[s]
        for s in new:
            nkf[s] += 1
    print("min_gap %d, min_matches %d: keyframes %s, accepted %s, skipped %s, candidate statuses %s" %
          (min_gap, min_matches, nkf, accepted, skipped, sorted(rc.STATUS_NAMES[t] for t in statuses)))
    assert min(nkf) >= 4
    assert {rc.FOUND, rc.NONE, rc.BAD_VECTOR} <= statuses
    for s in range(2):
        assert p.pose_graph_optimization([s])[0]["nedge"] == nkf[s] - 1 + accepted[s]      # an accepted pair is one more edge
        assert len(ref.read(s)[0]) == nkf[s] - accepted[s] - skipped[s] - (1 if s == 1 else 0)
    if min_gap == 1:
        assert sum(accepted) >= 1 and sum(skipped) >= 1
    p.close()


def test_refused_with_the_map_on_the_device(svs):
    pl = importlib.import_module("stereovision-slam_amd.pipeline")
    d = pl.Pipeline(pl.default_config(device_map=1), nstreams=1)
    for i in range(3):
        a, b = svs.synth_pair(SEEDS[0], i)
        d.step([a], [b])
    d.loopdb_configure(8, 16)
    with pytest.raises(RuntimeError, match="device"):
        d.detect_loops(np.ones((1, 16), np.float32))
    d.close()
