"""tests/ref_local_fusion.py on its own: properties the rules of LocalFusion must have whatever computes them.  CPU only."""
import numpy as np
import pytest

import local_fusion_cases as lc
import ref_local_fusion as rlf

IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)


def _state(w):
    return (np.array([w.map.active_keyframes[k].pose for k in sorted(w.map.active_keyframes)]),
            np.array([w.map.active_landmarks[i].pos for i in sorted(w.map.active_landmarks)]), w.last.pose.copy())


def _centre(T):
    return rlf.se3_inv(T)[4:]


@pytest.mark.parametrize("cur_active,last_is_kf", [(True, False), (True, True), (False, False)])
def test_the_identity_correction_leaves_everything_in_place(cur_active, last_is_kf):
    w = lc.scripted_window(1, cur_active=cur_active, last_is_kf=last_is_kf)
    poses, pts, last = _state(w)
    rel = [f.relative_pose_pkf.copy() for f in w.frames]
    st = rlf.local_fusion(w.map, w.last, w.cur, w.cand, w.cur.pose.copy(), [], frames=[w.last])
    poses2, pts2, last2 = _state(w)
    assert st["n_unanchored"] == 0 and st["npt"] == len(pts) > 20 and st["nkf"] == len(poses)
    assert np.abs(poses2 - poses).max() < 1e-13 and np.abs(pts2 - pts).max() < 1e-12 and np.abs(last2 - last).max() < 1e-13
    if cur_active:
        assert np.array_equal(w.cur.pose, poses[-1])              # corrected[cur] is T_corr itself, not a product
    assert all(np.array_equal(a, f.relative_pose_pkf) for a, f in zip(rel, w.frames))


@pytest.mark.parametrize("cur_active", [True, False])
def test_a_pure_translation_moves_window_and_landmarks_rigidly(cur_active):
    w = lc.scripted_window(2, cur_active=cur_active)
    poses, pts, last = _state(w)
    d = np.array([0.7, -0.3, 1.9])
    T_corr = rlf.se3_mul(w.cur.pose, np.concatenate([IDENT[:4], d]))          # the world shifted by d under every camera
    inactive_cur = w.cur.pose.copy()
    rlf.local_fusion(w.map, w.last, w.cur, w.cand, T_corr, [], frames=[w.last])
    poses2, pts2, last2 = _state(w)
    assert np.abs(pts2 - (pts - d)).max() < 1e-12
    for a, b in zip(poses, poses2):
        assert np.abs(a[:4] - b[:4]).max() < 1e-15 and np.abs(_centre(b) - (_centre(a) - d)).max() < 1e-12
    assert np.abs(_centre(last2) - (_centre(last) - d)).max() < 1e-12
    if not cur_active:
        assert np.array_equal(w.cur.pose, inactive_cur)          # step 4 writes the active keyframes only


@pytest.mark.parametrize("seed,cur_active", [(3, True), (4, False), (5, True)])
def test_fusion_does_not_move_any_reprojection(seed, cur_active):
    """the correction is one rigid motion of the window: every landmark lands on the same pixel of every window keyframe.
    A wrong association order, the new T_k in step 2 or the last observation instead of the first break this"""
    w = lc.scripted_window(seed, cur_active=cur_active)
    before = lc.reprojections(w)
    T_corr = rlf.se3_mul(lc.small_motion(w.rng, 0.2, 3.0), w.cur.pose)
    st = rlf.local_fusion(w.map, w.last, w.cur, w.cand, T_corr, [], frames=[w.last])
    assert st["n_unanchored"] == 0 and before.shape[1] > 20
    assert np.abs(lc.reprojections(w) - before).max() < 1e-9
    if cur_active:
        assert np.array_equal(w.cur.pose, T_corr)


def test_a_landmark_without_an_anchor_stays_and_is_counted():
    w = lc.scripted_window(6)
    i = sorted(w.map.active_landmarks)[3]
    mp = w.map.active_landmarks[i]
    for f in mp.observations:
        f.map_point = None                                        # no feature names a live landmark any more
    keep = mp.pos.copy()
    st = rlf.local_fusion(w.map, w.last, w.cur, w.cand, rlf.se3_mul(lc.small_motion(w.rng), w.cur.pose), [], frames=[w.last])
    assert st["n_unanchored"] == 1 and np.array_equal(mp.pos, keep)


def _pair(w):
    """(ci, qi, mp_loop, mp_curr): a candidate feature and a current feature with distinct live landmarks"""
    ci = next(i for i, f in enumerate(w.cand.feature_left) if f.map_point is not None)
    mp_loop = w.cand.feature_left[ci].map_point
    qi = next(i for i, f in enumerate(w.cur.feature_left) if f.map_point is not None and f.map_point is not mp_loop and f.map_point.observations)
    return ci, qi, mp_loop, w.cur.feature_left[qi].map_point


def test_replacement_moves_the_observations_and_deletes_the_current_landmark():
    w = lc.scripted_window(7)
    ci, qi, mp_loop, mp_curr = _pair(w)
    moved = list(mp_curr.observations)
    n0, t0 = len(mp_loop.observations), mp_loop.observed_times
    carried = [f for f in w.last.feature_left if f.map_point is mp_curr]
    st = rlf.local_fusion(w.map, w.last, w.cur, w.cand, w.cur.pose.copy(), [(ci, qi), (ci, qi)], frames=[w.last])
    assert st["pairs"] == 1 and st["merged"] == 1 and st["repointed"] == len(moved) and st["same_deleted"] == 0
    assert mp_loop.observations[n0:] == moved and mp_loop.observed_times == t0 + len(moved)
    assert all(f.map_point is mp_loop for f in moved)
    assert mp_curr.id not in w.map.landmarks and mp_curr.id not in w.map.active_landmarks
    assert all(f.map_point is None for f in carried)              # a tracked frame's pointer has expired
    assert (mp_loop.id in w.map.active_landmarks) == any(f.frame.keyframe_id >= 2 for f in mp_loop.observations[:n0])   # not made active


def test_the_same_landmark_on_both_sides_is_deleted():
    w = lc.scripted_window(8)
    ci, qi, mp_loop, _ = _pair(w)
    w.cur.feature_left[qi].map_point = mp_loop
    feats = [f for fr in w.frames for f in fr.feature_left + fr.feature_right if f.map_point is mp_loop]
    st = rlf.local_fusion(w.map, w.last, w.cur, w.cand, w.cur.pose.copy(), [(ci, qi)], frames=[w.last])
    assert st["same_deleted"] == 1 and st["merged"] == 0
    assert mp_loop.id not in w.map.landmarks and all(f.map_point is None for f in feats)


def test_expired_landmarks_on_either_side_and_the_set_s_order():
    w = lc.scripted_window(9)
    ci, qi, mp_loop, mp_curr = _pair(w)
    # mp_curr expired: the feature is pointed at mp_loop, no observation is added
    w.cur.feature_left[qi].map_point = None
    n0 = len(mp_loop.observations)
    st = rlf.local_fusion(w.map, w.last, w.cur, w.cand, w.cur.pose.copy(), [(ci, qi)], frames=[w.last])
    assert st["repointed"] == 1 and st["merged"] == 0 and w.cur.feature_left[qi].map_point is mp_loop and len(mp_loop.observations) == n0
    # mp_loop expired: nothing happens
    w2 = lc.scripted_window(9)
    ci, qi, mp_loop, mp_curr = _pair(w2)
    del w2.map.landmarks[mp_loop.id]
    st = rlf.local_fusion(w2.map, w2.last, w2.cur, w2.cand, w2.cur.pose.copy(), [(ci, qi)], frames=[w2.last])
    assert st["pairs"] == 1 and st["repointed"] == 0 and w2.cur.feature_left[qi].map_point is mp_curr and mp_curr.id in w2.map.landmarks
    # two pairs on one current feature, ascending (ci, qi): the first merges mp_curr into A, the second sees the feature naming A
    w3 = lc.scripted_window(9)
    ci, qi, mp_a, mp_curr = _pair(w3)
    cj = next(i for i, f in enumerate(w3.cand.feature_left) if i > ci and f.map_point is not None and f.map_point not in (mp_a, mp_curr))
    mp_b = w3.cand.feature_left[cj].map_point
    st = rlf.local_fusion(w3.map, w3.last, w3.cur, w3.cand, w3.cur.pose.copy(), [(cj, qi), (ci, qi)], frames=[w3.last])
    assert st["merged"] == 2 and mp_curr.id not in w3.map.landmarks and mp_a.id not in w3.map.landmarks
    assert w3.cur.feature_left[qi].map_point is mp_b
