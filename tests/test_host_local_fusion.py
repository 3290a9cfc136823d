"""The host glue of LocalFusion (Map::RemoveLandmark / Revive, Pipeline::LocalFusion, DetectLoops' local_fusion flag) on scripted maps:
tests/cpp/local_fusion_host.cpp with a CPU kernel provider whose local-fusion call is csrc/k_local_fusion.h compiled for the host.
The program checks its scenarios itself and writes the map before and after each fusion; here every `before` is loaded into
tests/ref_glue.py's object graph, tests/ref_local_fusion.py runs on it, and the result has to be the program's `after`: poses and
positions bit for bit, every feature's landmark, every landmark's counter, anchor and observation list exactly.  The program runs a
second time built with -fsanitize=address,undefined (stand-alone: it has its own main, nothing is preloaded).  No GPU."""
import os
import subprocess
import types

import numpy as np
import pytest

import ref_glue as rg
import ref_local_fusion as rlf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = ("merge_live", "revive", "revive_slid", "same_landmark", "curr_expired", "loop_expired", "two_pairs_one_feature", "cur_inactive",
             "detect_loops")


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    out = tmp_path / (name + "_out")
    out.mkdir()
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off"] + extra +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "local_fusion_host.cpp"), "-o", exe])
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all local-fusion host tests passed" in r.stdout
    return out, r


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("lf_host"), "local_fusion_host", [])[0]


def test_local_fusion_host_cpp_under_the_sanitizers(tmp_path):
    _, r = _build_and_run(tmp_path, "local_fusion_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def _tokens(text):
    return [[float.fromhex(t) if t.lstrip("-").startswith("0x") else t for t in line.split()] for line in text.splitlines()]


def _load(text):
    """the program's dump -> ref_glue's object graph"""
    ev = {"evict_nearest": 0, "evict_farthest": 0, "cleaned_landmarks": 0}
    m = rg.Map(3, ev)
    w = types.SimpleNamespace(map=m, last=None, motion=None, names={})
    cur = None
    mp_of = []                                        # (feature, landmark id) to link once the landmarks are read
    lm = None
    for t in _tokens(text):
        if t[0] in ("kf", "last"):
            cur = rg.Frame(int(t[1]), None, None)
            cur.pose = np.array(t[5:12]); cur.relative_pose_pkf = np.array(t[12:19])
            if t[0] == "kf":
                cur.is_keyframe, cur.keyframe_id = True, int(t[2])
                m.keyframes[cur.keyframe_id] = cur
                if t[3] == "1":
                    m.active_keyframes[cur.keyframe_id] = cur
            else:
                w.last = cur
        elif t[0] == "f":
            f = rg.Feature(cur, (0.0, 0.0)); f.outlier = t[3] == "1"
            cur.feature_left.append(f); mp_of.append((f, int(t[2])))
            if t[4] == "x":
                cur.feature_right.append(None)
            else:
                g = rg.Feature(cur, (0.0, 0.0)); g.is_on_left_image = False; g.outlier = t[5] == "1"
                cur.feature_right.append(g); mp_of.append((g, int(t[4])))
        elif t[0] == "lastkf":
            w.last = m.keyframes[int(t[1])]
        elif t[0] == "motion":
            w.motion = t
        elif t[0] == "lm":
            lm = rg.MapPoint(int(t[1]))
            lm.observed_times = int(t[3]); lm.pos = np.array(t[6:9])
            lm.first_valid_obs = types.SimpleNamespace(frame=m.keyframes[int(t[4])]) if int(t[4]) >= 0 else None
            m.landmarks[lm.id] = lm
            if t[2] == "1":
                m.active_landmarks[lm.id] = lm
        elif t[0] == "o":
            fr = m.keyframes[int(t[1])]
            lm.observations.append((fr.feature_left if t[3] == "1" else fr.feature_right)[int(t[2])])
    for f, i in mp_of:
        f.map_point = m.landmarks.get(i)
    return w


def _dump(w):
    """the graph in the program's format, as tokens"""
    m = w.map
    out = []

    def named(f):
        mp = rlf.lock(m, f.map_point)
        return str(mp.id) if mp is not None else "-1"

    def frame(fr, tag):
        out.append([tag, str(fr.id), str(fr.keyframe_id if fr.is_keyframe else -1), "1" if fr.is_keyframe and fr.keyframe_id in m.active_keyframes else "0",
                    str(len(fr.feature_left))] + [float(v) for v in fr.pose] + [float(v) for v in fr.relative_pose_pkf])
        for i, f in enumerate(fr.feature_left):
            g = fr.feature_right[i]
            out.append(["f", str(i), named(f), "1" if f.outlier else "0"] + (["x", "x"] if g is None else [named(g), "1" if g.outlier else "0"]))
    for k in sorted(m.keyframes):
        frame(m.keyframes[k], "kf")
    if w.last.is_keyframe:
        out.append(["lastkf", str(w.last.keyframe_id)])
    else:
        frame(w.last, "last")
    out.append(w.motion)
    for i in sorted(m.landmarks):
        mp = m.landmarks[i]
        a = getattr(mp, "first_valid_obs", None)
        out.append(["lm", str(i), "1" if i in m.active_landmarks else "0", str(mp.observed_times), str(a.frame.keyframe_id if a is not None else -1),
                    str(len(mp.observations))] + [float(v) for v in mp.pos])
        for f in mp.observations:
            fr = f.frame
            lst = fr.feature_left if f.is_on_left_image else fr.feature_right
            out.append(["o", str(fr.keyframe_id), str(next(k for k, g in enumerate(lst) if g is f)), "1" if f.is_on_left_image else "0"])
    return out


def test_the_loader_and_the_dump_are_inverse(dumps):
    for name in SCENARIOS:
        text = (dumps / (name + ".before")).read_text()
        assert _dump(_load(text)) == _tokens(text), name


@pytest.mark.parametrize("name", SCENARIOS)
def test_the_host_does_what_the_second_reading_does(dumps, name):
    w = _load((dumps / (name + ".before")).read_text())
    job = _tokens((dumps / (name + ".job")).read_text())
    kf, cand, T_corr = int(job[0][1]), int(job[0][2]), np.array(job[0][3:10])
    pairs = [(int(t[1]), int(t[2])) for t in job if t[0] == "pair"]
    stats = [int(v) for v in next(t for t in job if t[0] == "stats")[1:]]
    st = rlf.local_fusion(w.map, w.last, w.map.keyframes[kf], w.map.keyframes[cand], T_corr, pairs, frames=[w.last])
    got, want = _dump(w), _tokens((dumps / (name + ".after")).read_text())
    for a, b in zip(got, want):
        assert a == b, (name, a, b)
    assert len(got) == len(want)
    nkf, npt, unanchored, npairs, merged, revived, repointed, same = stats
    assert (st["nkf"], st["npt"], st["n_unanchored"], st["pairs"], st["merged"], st["repointed"], st["same_deleted"]) == \
        (nkf, npt, unanchored, npairs, merged, repointed, same), (st, stats)
    assert npt > 5 and nkf == 3
