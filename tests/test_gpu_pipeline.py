"""End-to-end: the C++ host pipeline over the HIP kernels (product) against its CPU
twin (same host logic over the oracle kernels) on the same synthetic stereo stream."""
import importlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _run(pipe, svs, seeds, nframes):
    est = np.zeros((nframes, len(seeds), 7)); meta = []
    for f in range(nframes):
        pairs = [svs.synth_pair(s, f) for s in seeds]
        res = pipe.step([p[0] for p in pairs], [p[1] for p in pairs])
        est[f] = res["pose"]
        meta.append(res.copy())
    return est, meta


def test_pipeline_matches_cpu_twin(svs, monkeypatch):
    import pipe_cpu
    pl = importlib.import_module("stereovision-slam_amd.pipeline")
    monkeypatch.setenv("SVS_ORACLE_BA_JAC", "0")   # analytic J on both sides: tight comparison
    seeds, N = [7, 8, 9], 30
    gpu = pl.Pipeline(nstreams=len(seeds))
    cpu = pipe_cpu.make(nstreams=len(seeds))
    eg, mg = _run(gpu, svs, seeds, N)
    ec, mc = _run(cpu, svs, seeds, N)
    # Integer-valued stages (GFTT, LK) are bit-exact, the f64 LM chains agree to rounding;
    # a chi2 that lands within rounding of 5.991 can flip one outlier bit, after which the
    # two runs are both valid but no longer identical ("reported mismatch
    # count").  So: the first 10 frames must match exactly, later frames may differ by a
    # few inliers, and the trajectories stay within centimetres (ATE difference < 1 cm).
    keys = ("status", "is_keyframe", "n_features", "n_inliers", "keyframe_id")
    for f in range(10):
        for k in keys:
            assert np.array_equal(mg[f][k], mc[f][k]), (f, k, mg[f][k], mc[f][k])
    # absolute poses: the local BA fixes no vertex (src/backend.cpp:39-66), so each call leaves a
    # 6-DoF gauge that only the LM damping pins; rounding differences move along it freely
    # (the per-call parity tests compare gauge-invariant quantities at 1e-6).  5e-4 m here.
    assert np.allclose(eg[:10, :, 4:], ec[:10, :, 4:], atol=5e-4), np.abs(eg[:10] - ec[:10]).max()
    assert np.allclose(eg[:10, :, :4], ec[:10, :, :4], atol=5e-5)
    mism = sum(int((mg[f][k] != mc[f][k]).sum()) for f in range(N) for k in keys)
    print("metadata mismatches after frame 10:", mism, "of", N * len(seeds) * len(keys))
    assert mism <= 0.1 * N * len(seeds) * len(keys)
    for f in range(N):
        assert np.array_equal(mg[f]["status"], mc[f]["status"])
        assert np.abs(mg[f]["n_inliers"] - mc[f]["n_inliers"]).max() <= 5
    # after a flip the two (equally valid) runs drift apart at the centimetre level of the ATE itself
    assert np.allclose(eg[..., 4:], ec[..., 4:], atol=5e-2), np.abs(eg - ec).max()
    for k, sd in enumerate(seeds):
        gt = np.array([svs.synth_gt(sd, f) for f in range(N)])
        assert abs(pl.ate_rmse(eg[:, k], gt) - pl.ate_rmse(ec[:, k], gt)) < 1e-2
    cg, cc = gpu.counters(), cpu.counters()
    assert abs(cg["keyframes"] - cc["keyframes"]) <= 1
    assert cg["keyframes"] >= 3 * 3 and cg["ba_calls"] == cg["keyframes"]
    gpu.close(); cpu.close()


def test_pipeline_ate_vs_reference_faithful_twin(svs):
    """GPU path (analytic BA Jacobians) vs the twin with g2o-style numeric Jacobians:
    ATE against ground truth within 1% of each other (north_star), and small."""
    import pipe_cpu
    pl = importlib.import_module("stereovision-slam_amd.pipeline")
    os.environ.pop("SVS_ORACLE_BA_JAC", None)
    seeds, N = [21], 60
    gpu = pl.Pipeline(nstreams=1)
    cpu = pipe_cpu.make(nstreams=1)
    eg, _ = _run(gpu, svs, seeds, N)
    ec, _ = _run(cpu, svs, seeds, N)
    gt = np.array([svs.synth_gt(seeds[0], f) for f in range(N)])
    ag, ac = pl.ate_rmse(eg[:, 0], gt), pl.ate_rmse(ec[:, 0], gt)
    assert ag < 0.25 and ac < 0.25, (ag, ac)
    # 1% of the ATE (north_star) with a 5 mm floor: on a 50 m path the ATE itself is ~2 cm and
    # two valid runs differ by millimetres once an outlier bit flips (see the test above)
    assert abs(ag - ac) <= 0.01 * ac + 5e-3, (ag, ac)
    gpu.close(); cpu.close()


def test_pipeline_backend_beside_frontend_matches_cpu_twin(svs, monkeypatch):
    """backend_on == 2: local BA submitted on a second context, collected one frame later."""
    import pipe_cpu
    pl = importlib.import_module("stereovision-slam_amd.pipeline")
    monkeypatch.setenv("SVS_ORACLE_BA_JAC", "0")
    seeds, N = [7, 8, 9], 24
    cfg = pl.default_config(backend_on=2)
    gpu = pl.Pipeline(cfg, nstreams=len(seeds))
    cpu = pipe_cpu.make(cfg, nstreams=len(seeds))
    assert gpu.backend_ctx() != gpu.kernel_ctx()
    eg, mg = _run(gpu, svs, seeds, N)
    ec, mc = _run(cpu, svs, seeds, N)
    gpu.flush(); cpu.flush()
    keys = ("status", "is_keyframe", "n_features", "n_inliers", "keyframe_id")
    for f in range(10):
        for k in keys:
            assert np.array_equal(mg[f][k], mc[f][k]), (f, k, mg[f][k], mc[f][k])
    assert np.allclose(eg[:10, :, 4:], ec[:10, :, 4:], atol=5e-4), np.abs(eg[:10] - ec[:10]).max()
    assert np.allclose(eg[..., 4:], ec[..., 4:], atol=5e-2), np.abs(eg - ec).max()
    cg, cc = gpu.counters(), cpu.counters()
    assert cg["ba_calls"] == cg["keyframes"] and abs(cg["keyframes"] - cc["keyframes"]) <= 1   # flushed
    for k, sd in enumerate(seeds):
        gt = np.array([svs.synth_gt(sd, f) for f in range(N)])
        assert pl.ate_rmse(eg[:, k], gt) < 0.1
    gpu.close(); cpu.close()


def test_pipeline_full_resolution_input(svs):
    """f3 on the product path: 1241x376 frames resident in host memory, decimation fused into
    level 0 (svslam_set_source_size) == the same pipeline fed with pre-decimated frames."""
    pl = importlib.import_module("stereovision-slam_amd.pipeline")
    SW, SH = 1241, 376
    cam2 = tuple(2 * v for v in svs.KITTI00_HALF_CAM)
    full = [svs.synth_pair(4, f, SW, SH, cam2) for f in range(8)]
    half = [(l[::2, ::2][:188, :620].copy(), r[::2, ::2][:188, :620].copy()) for l, r in full]
    a = pl.Pipeline(pl.default_config(src_width=SW, src_height=SH), nstreams=1)
    b = pl.Pipeline(nstreams=1)
    for (fl, fr), (hl, hr) in zip(full, half):
        ra = a.step([fl], [fr]); rb = b.step([hl], [hr])
        assert np.array_equal(ra["pose"], rb["pose"]) and ra["n_features"][0] == rb["n_features"][0]
    a.close(); b.close()


def test_pipeline_backend_off_frontend_only_matches_cpu_twin(svs):
    """BASELINE config 2: HIP frontend with the backend switched off (backend_on = 0, config-00.yaml's
    key).  Per call the kernels are bit-exact (LK, GFTT) or agree to rounding (pose LM), but LK's
    stopping rule makes a frame's output discontinuous in its f32 initial guesses, so a 1e-13 pose
    difference grows ~100x per frame until it saturates at the LK tolerance (0.01 px, millimetres of
    pose): the first frames must match exactly, later ones within that noise floor."""
    import pipe_cpu
    pl = importlib.import_module("stereovision-slam_amd.pipeline")
    seeds, N = [11, 12], 24
    cfg = pl.default_config(backend_on=0)
    gpu = pl.Pipeline(cfg, nstreams=len(seeds))
    cpu = pipe_cpu.make(cfg, nstreams=len(seeds))
    eg, mg = _run(gpu, svs, seeds, N)
    ec, mc = _run(cpu, svs, seeds, N)
    for f in range(5):
        for k in ("status", "is_keyframe", "n_features", "n_inliers", "keyframe_id"):
            assert np.array_equal(mg[f][k], mc[f][k]), (f, k, mg[f][k], mc[f][k])
    assert np.allclose(eg[:4], ec[:4], atol=1e-5), np.abs(eg[:4] - ec[:4]).max()
    for f in range(N):
        assert np.array_equal(mg[f]["status"], mc[f]["status"])
        assert np.abs(mg[f]["n_features"] - mc[f]["n_features"]).max() <= 4
        assert np.abs(mg[f]["n_inliers"] - mc[f]["n_inliers"]).max() <= 4
    assert np.allclose(eg[..., 4:], ec[..., 4:], atol=2e-2), np.abs(eg - ec).max()
    assert gpu.counters()["ba_calls"] == 0 and gpu.counters()["keyframes"] >= 4
    for k, sd in enumerate(seeds):
        gt = np.array([svs.synth_gt(sd, f) for f in range(N)])
        assert abs(pl.ate_rmse(eg[:, k], gt) - pl.ate_rmse(ec[:, k], gt)) < 1e-2
    gpu.close(); cpu.close()


def test_pipeline_seq05_shape_seven_keyframe_window(svs, monkeypatch):
    """BASELINE config 3: KITTI-05-shaped input (1226x370 -> 613x185: odd width, so the generic
    pyramid kernels and unaligned rows are on the path) with local BA over the last 7 keyframes."""
    import pipe_cpu
    pl = importlib.import_module("stereovision-slam_amd.pipeline")
    monkeypatch.setenv("SVS_ORACLE_BA_JAC", "0")
    W, H = 613, 185
    cam = (353.5455, 353.5455, 300.9435, 91.55515)      # KITTI-05 calibration after the 1/2 scaling
    cfg = pl.default_config(W, H, cam=cam, num_active_keyframes=7)
    seeds, N = [31, 32], 60       # ~9 keyframes per stream: the 7-keyframe window slides
    gpu = pl.Pipeline(cfg, nstreams=len(seeds))
    cpu = pipe_cpu.make(cfg, nstreams=len(seeds))
    est = {}
    for name, pipe in (("gpu", gpu), ("cpu", cpu)):
        e = np.zeros((N, len(seeds), 7)); meta = []
        for f in range(N):
            pairs = [svs.synth_pair(s, f, W, H, cam) for s in seeds]
            res = pipe.step([p[0] for p in pairs], [p[1] for p in pairs])
            e[f] = res["pose"]; meta.append(res.copy())
        est[name] = (e, meta)
    (eg, mg), (ec, mc) = est["gpu"], est["cpu"]
    for f in range(8):
        for k in ("status", "is_keyframe", "n_features", "n_inliers", "keyframe_id"):
            assert np.array_equal(mg[f][k], mc[f][k]), (f, k, mg[f][k], mc[f][k])
    assert np.allclose(eg[:8, :, 4:], ec[:8, :, 4:], atol=5e-4), np.abs(eg[:8] - ec[:8]).max()
    cg = gpu.counters()
    assert cg["keyframes"] >= 2 * 8 and cg["ba_calls"] == cg["keyframes"]
    assert cg["ba_kf"] <= 7 * cg["ba_calls"]
    # 60 frames (~52 m): after the first flipped outlier bit the two runs are different, equally
    # valid SLAM runs (keyframes may fall one frame apart); they must agree at the level of the
    # trajectory error itself
    for k, sd in enumerate(seeds):
        gt = np.array([svs.synth_gt(sd, f) for f in range(N)])
        ag, ac = pl.ate_rmse(eg[:, k], gt), pl.ate_rmse(ec[:, k], gt)
        assert ag < 0.15 and ac < 0.15 and abs(ag - ac) < 3e-2, (ag, ac)
        assert pl.ate_rmse(eg[:, k], ec[:, k]) < 8e-2
    gpu.close(); cpu.close()


def test_pipeline_low_latency_shape_matches_cpu_twin(svs):
    """low_latency = 1 (svslam_set_low_latency: four wavefronts per pose-only job): same bounds as the
    default shape against the CPU twin, and deterministic."""
    import pipe_cpu
    pl = importlib.import_module("stereovision-slam_amd.pipeline")
    seeds, N = [41], 16
    cfg = pl.default_config(low_latency=1)
    a = pl.Pipeline(cfg, nstreams=1); b = pl.Pipeline(cfg, nstreams=1)
    cpu = pipe_cpu.make(pl.default_config(), nstreams=1)
    ea, ma = _run(a, svs, seeds, N)
    eb, _ = _run(b, svs, seeds, N)
    ec, mc = _run(cpu, svs, seeds, N)
    assert np.array_equal(ea, eb)
    for f in range(5):
        for k in ("status", "is_keyframe", "n_features", "n_inliers", "keyframe_id"):
            assert np.array_equal(ma[f][k], mc[f][k]), (f, k, ma[f][k], mc[f][k])
    assert np.allclose(ea[:4], ec[:4], atol=1e-5)
    assert np.allclose(ea[..., 4:], ec[..., 4:], atol=2e-2), np.abs(ea - ec).max()
    a.close(); b.close(); cpu.close()


def test_bench_contract_small_run():
    """bench.py --full prints exactly one JSON line with the driver's keys plus roofline and cpu_baseline."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "3",
                          "--streams", "16", "--groups", "2", "--host-threads", "1", "--cpu-frames", "40", "--full"],
                         capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 3 and d["unit"] == "frames/s"
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert abs(d["value"] - 16 * 6 / (d["ms_per_step"] * 6e-3)) <= 1e-3 * d["value"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-6 and r["achieved"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and c["unit"] == "frames/s" and c["sample"]
    assert "workload" in d["config"] and d["config"]["checks"]["duplicate_stream_bit_identical"] is True
    # the timed region is the steady state whatever --warmup / --steps are: the pre-roll ran until the
    # sliding window of local BA was full
    assert d["config"]["preroll_steps"] >= 60 and d["config"]["ba_problem_mean"]["keyframes"] >= 9.5
    assert r["peak_measured"] == 6290.0
    # round 6: the reported run is the configuration BASELINE.json's metric names — 1241x376 frames in HBM, the 1/2 decimation fused
    # — and its roofline object prices ONE kernel, named, with the stamp of the PMC summary its traffic figure comes from
    assert d["config"]["frame"].startswith("1241x376") and "frame_ring" in d["config"]
    assert r["interval"] in ("ba_solve", "pyramid", "lk", "pose_only", "gftt", "triangulate") and r["kernel"].startswith("k_")
    assert set(d["kernel_ms"]) >= {"pyramid", "lk", "gftt", "triangulate", "pose_only", "local_ba", "ba_solve"}
    assert d["kernel_ms"]["ba_solve"] <= d["kernel_ms"]["local_ba"]
    assert " src " in d["library"] and set(d["pmc_stamps"]) == {"pmc_traffic.json", "pmc_valu.json", "pmc_valu_step.json"}
    assert isinstance(r["traffic_stamp"]["matches_loaded_library"], bool)
    assert d["value_super_window"]["steps"] == 36 and d["value_super_window"]["value"] > 0
    a = d["cpu_baseline_all_cores"]
    assert a["kind"] == "port" and a["cores"] >= 1 and a["value"] >= 0.8 * c["value"]


def test_bench_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """bench.py without --full: one JSON line with the headline keys and none of the --full legs; the timed window is exactly
    --steps steps; --dump-outputs writes the per-stream results of the last timed step (float64, stream order), and two runs
    with the same arguments dump the same arrays."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    S, K, Wm = 16, 5, 2
    fields = ("pose", "status", "is_keyframe", "n_features", "n_inliers", "frame_id", "keyframe_id")
    dumps = []
    for i in range(2):
        d = tmp_path / ("run%d" % i)
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(Wm),
                              "--streams", str(S), "--groups", "2", "--host-threads", "1", "--dump-outputs", str(d)],
                             capture_output=True, text=True, timeout=600, cwd=root)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        r = json.loads(lines[0])
        assert r["steps"] == K and r["warmup"] == Wm and r["unit"] == "frames/s" and r["higher_is_better"] is True
        assert r["metric"].startswith("stereo frames/sec") and r["dtype"].startswith("u8/i32")
        assert abs(r["value"] - S * K / (r["ms_per_step"] * K * 1e-3)) <= 1e-3 * r["value"]
        for k in ("roofline", "kernel_ms", "cpu_baseline", "value_windows", "value_spread", "value_super_window", "host_ms_per_step"):
            assert k not in r, k
        assert "checks" not in r["config"] and r["config"]["streams_per_gpu"] == S
        a = {f: np.load(str(d / (f + ".npy"))) for f in fields}
        assert sorted(os.listdir(d)) == sorted(f + ".npy" for f in fields)
        assert all(v.dtype == np.float64 and len(v) == S for v in a.values()) and a["pose"].shape == (S, 7)
        assert (a["frame_id"] == r["config"]["preroll_steps"] + Wm + K - 1).all()
        assert np.array_equal(a["pose"][0], a["pose"][S // 2])     # the duplicated stream (first of the second group)
        dumps.append(a)
    for f in fields:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f


def test_sampled_render_is_the_full_render_where_the_decimation_samples(svs):
    """synth_render_streams_device(sampled=True), what bench.py renders its full-size frames with: the pixels (2x, 2y) are those of
    a full render and each fills its 2x2 block (1241 columns: the last sampled column has no right neighbour)"""
    SW, SH, F = 1241, 376, 2
    seeds = [11, 12, 13]
    cam2 = tuple(2 * v for v in svs.KITTI00_HALF_CAM)
    ctx = svs.Context(620, 188, max_slots=1, max_jobs=1)
    bufs = [ctx.dev_alloc(len(seeds) * F * SW * SH) for _ in range(4)]
    svs.synth_render_streams_device(seeds, 5, F, SW, SH, bufs[0], bufs[1], cam=cam2)
    svs.synth_render_streams_device(seeds, 5, F, SW, SH, bufs[2], bufs[3], cam=cam2, sampled=True)
    imgs = []
    for b in bufs:
        a = np.zeros((len(seeds) * F, SH, SW), np.uint8)
        ctx.dev_download(b, a)
        imgs.append(a)
        ctx.dev_free(b)
    ctx.close()
    for full, smp in ((imgs[0], imgs[2]), (imgs[1], imgs[3])):
        kept = full[:, ::2, ::2]
        assert np.array_equal(smp[:, ::2, ::2], kept)
        assert np.array_equal(smp, np.repeat(np.repeat(kept, 2, 1), 2, 2)[:, :SH, :SW])


def test_pipeline_config2_hip_frontend_with_cpu_backend(svs):
    """BASELINE config 2 as written: HIP GFTT + LK (+ triangulation, pose-only) frontend with the
    backend still on the CPU (the oracle's g2o-shaped BA, numeric Jacobians).  Against the full CPU
    twin the only difference left is the frontend, whose integer stages are bit-exact: metadata must
    agree for the first frames and the trajectories stay within the LK noise floor."""
    import pipe_cpu
    pl = importlib.import_module("stereovision-slam_amd.pipeline")
    os.environ.pop("SVS_ORACLE_BA_JAC", None)
    seeds, N = [7, 8], 30
    hyb = pipe_cpu.make_hybrid(nstreams=len(seeds))
    cpu = pipe_cpu.make(nstreams=len(seeds))
    assert hyb.kernel_ctx()                       # really the HIP provider
    eh, mh = _run(hyb, svs, seeds, N)
    ec, mc = _run(cpu, svs, seeds, N)
    keys = ("status", "is_keyframe", "n_features", "n_inliers", "keyframe_id")
    for f in range(10):
        for k in keys:
            assert np.array_equal(mh[f][k], mc[f][k]), (f, k, mh[f][k], mc[f][k])
    # both sides run the numeric-Jacobian BA (delta = 1e-9, like g2o): its noise moves the solution along
    # the 6 gauge directions no vertex pins, so rounding-level differences of the frontends show up as
    # millimetres of ABSOLUTE pose (gauge-invariant quantities agree far better, see the per-call tests)
    assert np.allclose(eh[:10, :, 4:], ec[:10, :, 4:], atol=5e-3), np.abs(eh[:10] - ec[:10]).max()
    assert np.allclose(eh[..., 4:], ec[..., 4:], atol=5e-2), np.abs(eh - ec).max()
    ch, cc = hyb.counters(), cpu.counters()
    assert ch["ba_calls"] == ch["keyframes"] and abs(ch["keyframes"] - cc["keyframes"]) <= 1
    for k, sd in enumerate(seeds):
        gt = np.array([svs.synth_gt(sd, f) for f in range(N)])
        assert abs(pl.ate_rmse(eh[:, k], gt) - pl.ate_rmse(ec[:, k], gt)) < 1e-2
    hyb.close(); cpu.close()


@pytest.mark.parametrize("device_map", [0, 1])
def test_hip_pipeline_meets_the_second_reading_of_the_glue(svs, device_map):
    """tests/golden/glue_second_reading.npz holds what tests/ref_glue.py — the plain-Python restatement of the reference's
    Frontend / Map / MapPoint / Backend glue, written from /root/reference alone — reports and holds after
    every frame of two seeded streams.  The HIP pipeline must meet it: the first frames exactly (status, keyframe flag, feature and
    inlier counts, ids; with the map on the host also the active window, the landmark count, the observation total and the
    checksum of every observation list), poses to LM tolerance; later frames: same status, same keyframe count (+- 1), same
    trajectory error (the flipped outlier bits of test_pipeline_matches_cpu_twin)."""
    import glue_scenarios as gs
    pl = importlib.import_module("stereovision-slam_amd.pipeline")
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "glue_second_reading.npz"))
    N = g["status"].shape[1]
    keys = ("status", "is_keyframe", "n_features", "n_inliers", "frame_id", "keyframe_id")
    for si, seed in enumerate(int(v) for v in g["seeds"]):
        pipe = pl.Pipeline(pl.default_config(device_map=device_map), nstreams=1)
        mism = 0
        est = np.zeros((N, 7))
        for f, (left, right) in enumerate(gs.frames(seed, "plain", N)):
            r = pipe.step([left], [right])[0]
            for k in keys:
                same = int(r[k]) == int(g[k][si, f])
                assert same or f >= 10, (hex(seed), f, k, int(r[k]), int(g[k][si, f]))
                mism += 0 if same else 1
            est[f] = r["pose"]
            if f < 10:
                assert np.allclose(r["pose"][4:], g["pose"][si, f, 4:], atol=5e-4) and np.allclose(r["pose"][:4], g["pose"][si, f, :4], atol=5e-5), (hex(seed), f)
            assert int(r["status"]) == int(g["status"][si, f])
            if device_map == 0 and f < 10:
                kf, nlm, nobs, crc = gs.map_digest(pipe.map_snapshot(0))
                assert kf == [int(v) for v in g["window"][si, f] if v >= 0], (hex(seed), f, kf)
                assert (nlm, nobs, crc) == (int(g["n_landmarks"][si, f]), int(g["n_observations"][si, f]), int(g["map_crc32"][si, f])), (hex(seed), f)
        print("second-reading fixture, seed %d, device_map %d: %d of %d metadata values differ after frame 10" % (seed, device_map, mism, N * len(keys)))
        # (no bound on the count: once a keyframe falls one frame apart every later keyframe id and flag differs)
        kf_hip, kf_fix = int(pipe.counters()["keyframes"]), int(g["is_keyframe"][si].sum())
        assert abs(kf_hip - kf_fix) <= 1, (kf_hip, kf_fix)
        # after a flipped outlier bit the two runs are different, equally valid runs (the absolute pose then drifts along the gauge
        # the unpinned local BA leaves free — decimetres over these 50 m): they agree at the level of the trajectory error itself
        gt = np.array([svs.synth_gt(seed, f) for f in range(N)])
        a_hip, a_fix = pl.ate_rmse(est, gt), pl.ate_rmse(g["pose"][si], gt)
        assert a_hip < 0.15 and abs(a_hip - a_fix) < 2e-2, (a_hip, a_fix)
        pipe.close()
