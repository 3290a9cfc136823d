"""Colour input of the dense program on the device: svslam_pyramid_bgr_batch (k_bgr_prepare + the unchanged pyramid path),
svslam_colour_read, svslam_dense_cloud_bgr_batch (k_colour_gather behind the unchanged k_dense_cloud).

The yardsticks: tests/ref_colour.py for the grey image and the plane; the slot is compared with a second slot that
Context.pyramid builds from the numpy grey, in every level and with the stored border; the cloud with Context.dense_cloud on
such slots; the colours with the numpy plane indexed at pix.  Every refusal is a host-side argument check: nothing is launched."""
import ctypes as C

import numpy as np
import pytest

import common
import ref_colour as rc
import ref_stereo_bm as rsb
from colour_cases import DEC_DOWN, DEC_UP, DIRECT, KITTI, stereo_pair, strided

BASELINE = 0.537166


def _kitti_cam(w, h):
    return (718.856 * 0.5 * w / 620.0, 718.856 * 0.5 * w / 620.0, 0.5 * w, 0.5 * h)


_pairs = {}


def pair(case, seed=11):
    """(left, right, grey_left, grey_right, plane_left) of a case, computed once and left unchanged"""
    key = (case[0], seed)
    if key not in _pairs:
        (sw, sh), (w, h), disp, _ = case
        l, r = stereo_pair(seed, (sw, sh), disp)
        gl, pl = rc.prepare(l, w, h)
        gr, _ = rc.prepare(r, w, h)
        for a in (l, r, gl, gr, pl):
            a.setflags(write=False)
        _pairs[key] = (l, r, gl, gr, pl)
    return _pairs[key]


def _levels(ctx, slot):
    out = []
    for l in range(8):
        try:
            out.append(ctx.pyramid_read(slot, l))
        except RuntimeError:
            break
    return out


def _same_slot(ctx, a, b):
    la, lb = _levels(ctx, a), _levels(ctx, b)
    assert len(la) == len(lb) >= 2
    for l, (x, y) in enumerate(zip(la, lb)):
        assert np.array_equal(x, y), "level %d" % l
    for l in (0, len(la) - 1):
        assert np.array_equal(ctx.pyramid_read_padded(a, l), ctx.pyramid_read_padded(b, l)), "padded level %d" % l


def _ctx(svs, case, **kw):
    w, h = case[1]
    args = dict(max_slots=12, max_jobs=8, max_pts=8, max_corners=8, max_kf=0, max_lm=0, max_obs=0)
    args.update(kw)
    return svs.Context(w, h, **args)


@pytest.mark.gpu
@pytest.mark.parametrize("case,extra", [(DIRECT, 0), (DIRECT, 5), (DEC_DOWN, 0), (DEC_UP, 0), (KITTI, 0)])
def test_slot_and_plane_equal_the_grey_pyramid_and_the_numpy_plane(svs, case, extra):
    l, r, gl, gr, pl = pair(case)
    gr_plane = rc.prepare(r, *case[1])[1]
    c = _ctx(svs, case)
    try:
        c.colour_reserve(3)
        imgs = [strided(l, extra), strided(r, extra)] if extra else [l, r]
        c.pyramid_bgr([0, 1], [1, 2], imgs)
        c.pyramid([2, 3], [gl, gr])
        _same_slot(c, 0, 2)
        _same_slot(c, 1, 3)
        assert np.array_equal(c.colour_read(1), pl) and np.array_equal(c.colour_read(2), gr_plane)
        assert (pl[..., 0] != pl[..., 1]).mean() > 0.9            # a colour image: the channels differ
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case,extra", [(DIRECT, 5), (DEC_UP, 0), (DEC_DOWN, 3)])
def test_device_resident_sources_each_in_an_allocation_of_exactly_its_size(svs, case, extra):
    l, r, gl, gr, pl = pair(case)
    (sw, sh) = case[0]
    stride = 3 * sw + extra
    nbytes = stride * (sh - 1) + 3 * sw               # the bytes the ABI promises to stay within
    c = _ctx(svs, case)
    ptrs = []
    try:
        c.colour_reserve(2)
        for img in (l, r):
            buf = np.full(stride * sh, 0x5A, np.uint8)
            buf.reshape(sh, stride)[:, :3 * sw] = img.reshape(sh, 3 * sw)
            p = c.dev_alloc(nbytes)
            ptrs.append(p)
            c.dev_upload(p, buf[:nbytes])
        c.pyramid_bgr([4, 5], [0, -1], [(ptrs[0], sh, sw), (ptrs[1], sh, sw)], device=True, strides=[stride, stride])
        c.pyramid([2, 3], [gl, gr])
        _same_slot(c, 4, 2)
        _same_slot(c, 5, 3)
        assert np.array_equal(c.colour_read(0), pl)
    finally:
        for p in ptrs:
            c.dev_free(p)
        c.close()


@pytest.mark.gpu
def test_plane_bookkeeping_scrambled_planes_and_uploads_that_keep_no_colour(svs):
    (w, h) = DIRECT[1]
    rng = np.random.default_rng(23)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(8)]
    planes = [5, -1, 0, 3, -1, 1, 4, 2]
    c = _ctx(svs, DIRECT)
    try:
        c.colour_reserve(7)
        c.pyramid_bgr([0, 1, 2, 3, 4, 5, 6, 7], planes, imgs)
        c.pyramid([8], [rc.grey_from_bgr(imgs[6])])
        _same_slot(c, 6, 8)
        before = {}
        for i, p in enumerate(planes):
            if p >= 0:
                before[p] = c.colour_read(p)
                assert np.array_equal(before[p], imgs[i]), (i, p)
        # a later upload to other slots that keeps no colour leaves every plane as it was (plane 6 was never written: not compared)
        others = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(3)]
        c.pyramid_bgr([9, 10, 11], [-1, -1, -1], others)
        for p, img in before.items():
            assert np.array_equal(c.colour_read(p), img), p
        c.pyramid([8], [rc.grey_from_bgr(others[2])])
        _same_slot(c, 11, 8)
        # the same count keeps the contents, a new count drops them
        c.colour_reserve(7)
        assert np.array_equal(c.colour_read(5), imgs[0])
        c.colour_reserve(2)
        with pytest.raises(RuntimeError, match="has not been written"):
            c.dense_cloud_bgr([(0, 1, 0, None)], _kitti_cam(w, h), svs.IDENT, BASELINE, num_disparities=32, block_size=5)
    finally:
        c.close()


IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)


def _rigs(w, h):
    """(cam_l, ext_l, T_cw): the KITTI rig at the identity, a general rig (fx != fy, rotated extrinsic) at a general pose"""
    T = common.random_pose(np.random.default_rng(4), trans=0.3, rot=0.04)
    return {"kitti": (_kitti_cam(w, h), IDENT, None), "general": (common.GENERAL_RIG[0], common.GENERAL_RIG[1], T)}


@pytest.mark.gpu
@pytest.mark.parametrize("rig", ["kitti", "general"])
@pytest.mark.parametrize("case", [DIRECT, DEC_DOWN], ids=["97x53", "401x121"])
def test_coloured_cloud_equals_dense_cloud_and_the_plane_at_pix(svs, case, rig):
    l, r, gl, gr, pl = pair(case)
    w, h = case[1]
    nd, bs = case[3]
    cam, ext, T = _rigs(w, h)[rig]
    # the yardstick's own cloud: not empty, and of the size the device returns
    want_xyz, want_pix = rsb.dense_cloud(rsb.stereo_bm(gl, gr, nd, bs), cam, ext, BASELINE, IDENT if T is None else T)
    assert len(want_pix) > 100
    c = _ctx(svs, case)
    try:
        c.colour_reserve(4)
        c.pyramid_bgr([0, 1], [2, -1], [l, r])
        c.pyramid([2, 3], [gl, gr])
        (rx, rp, rd), = c.dense_cloud([(2, 3, T)], cam, ext, BASELINE, num_disparities=nd, block_size=bs)
        (gx, gp, gb, gd), = c.dense_cloud_bgr([(0, 1, 2, T)], cam, ext, BASELINE, num_disparities=nd, block_size=bs)
        assert np.array_equal(rp, want_pix) and len(gp) == len(want_pix)
        assert np.array_equal(gx, rx) and np.array_equal(gp, rp) and np.array_equal(gd, rd)
        assert gx.tobytes() == rx.tobytes()
        assert np.array_equal(gb, pl.reshape(-1, 3)[gp])
        assert ((gb[:, 0] != gb[:, 1]) | (gb[:, 1] != gb[:, 2])).any()
        # max_pts_per_job exactly at the count passes; one below is the error it is without colour
        n = len(gp)
        (_, p2, b2, _), = c.dense_cloud_bgr([(0, 1, 2, T)], cam, ext, BASELINE, max_pts_per_job=n, num_disparities=nd, block_size=bs)
        assert np.array_equal(p2, gp) and np.array_equal(b2, gb)
        msgs = []
        for call in (lambda: c.dense_cloud([(2, 3, T)], cam, ext, BASELINE, max_pts_per_job=n - 1, num_disparities=nd, block_size=bs),
                     lambda: c.dense_cloud_bgr([(0, 1, 2, T)], cam, ext, BASELINE, max_pts_per_job=n - 1, num_disparities=nd, block_size=bs)):
            with pytest.raises(RuntimeError, match="points > max_pts_per_job") as e:
                call()
            msgs.append(str(e.value).split(": ", 1)[1])
        assert msgs[0] == msgs[1]
    finally:
        c.close()


@pytest.mark.gpu
def test_three_jobs_whose_planes_are_not_their_job_indices(svs):
    w, h = DIRECT[1]
    nd, bs = DIRECT[3]
    cam = _kitti_cam(w, h)
    sets = [pair(DIRECT, seed) for seed in (11, 12, 13)]
    plane_of = [2, 0, 1]
    c = _ctx(svs, DIRECT)
    try:
        c.colour_reserve(3)
        c.pyramid_bgr([0, 1, 2, 3, 4, 5], [plane_of[0], -1, plane_of[1], -1, plane_of[2], -1], [s[k] for s in sets for k in (0, 1)])
        c.pyramid([6, 7, 8, 9, 10, 11], [s[k] for s in sets for k in (2, 3)])
        ref = c.dense_cloud([(6, 7, None), (8, 9, None), (10, 11, None)], cam, svs.IDENT, BASELINE, num_disparities=nd, block_size=bs)
        got = c.dense_cloud_bgr([(0, 1, plane_of[0], None), (2, 3, plane_of[1], None), (4, 5, plane_of[2], None)], cam, svs.IDENT, BASELINE,
                                num_disparities=nd, block_size=bs)
        for j, ((rx, rp, rd), (gx, gp, gb, gd)) in enumerate(zip(ref, got)):
            assert len(gp) > 100
            assert np.array_equal(gx, rx) and np.array_equal(gp, rp) and np.array_equal(gd, rd)
            assert np.array_equal(gb, sets[j][4].reshape(-1, 3)[gp]), j
            for k in range(3):
                if k != j and len(sets[k][4].reshape(-1, 3)[gp]) == len(gb):
                    assert not np.array_equal(gb, sets[k][4].reshape(-1, 3)[gp])      # another job's plane would show
    finally:
        c.close()


def _raw_upload(c, n, slots, planes, imgs, strides, sw, sh, device=0):
    arr = lambda v: None if v is None else (C.c_int * len(v))(*v)
    ptrs = None if imgs is None else (C.c_void_p * len(imgs))(*[None if im is None else im.ctypes.data for im in imgs])
    rc_ = c.L.svslam_pyramid_bgr_batch(c.h, n, arr(slots), arr(planes), ptrs, arr(strides), sw, sh, device)
    return rc_, c.L.svslam_last_error(c.h).decode()


@pytest.mark.gpu
def test_refusals_are_decided_on_the_host_and_change_nothing(svs):
    l, r, gl, gr, pl = pair(DIRECT)
    w, h = DIRECT[1]
    nd, bs = DIRECT[3]
    cam = _kitti_cam(w, h)
    c = _ctx(svs, DIRECT, max_slots=4, max_jobs=2)
    try:
        c.colour_reserve(3)
        c.pyramid_bgr([0, 1], [0, -1], [l, r])

        def good():
            (x, p, b, d), = c.dense_cloud_bgr([(0, 1, 0, None)], cam, svs.IDENT, BASELINE, num_disparities=nd, block_size=bs)
            return x.tobytes(), p.tobytes(), b.tobytes(), d.tobytes(), c.colour_read(0).tobytes(), c.pyramid_read_padded(0, 0).tobytes()
        first = good()
        other = np.ascontiguousarray(l[::-1])            # what a refused upload must not leave anywhere
        st = [3 * w, 3 * w]
        big = np.zeros((2 * h + 1, 2 * w + 3, 3), np.uint8)
        uploads = [
            ("null argument", (2, None, [0, 1], [other, other], st, w, h)),
            ("null argument", (2, [0, 1], None, [other, other], st, w, h)),
            ("null argument", (2, [0, 1], [0, 1], None, st, w, h)),
            ("null argument", (2, [0, 1], [0, 1], [other, other], None, w, h)),
            ("image 1 is null", (2, [0, 1], [0, 1], [other, None], st, w, h)),
            ("> max_jobs", (3, [0, 1, 2], [0, 1, 2], [other, other, other], st + [3 * w], w, h)),
            ("slot 4 out of range", (2, [0, 4], [0, 1], [other, other], st, w, h)),
            ("slot -1 out of range", (2, [-1, 1], [0, 1], [other, other], st, w, h)),
            ("plane 3 out of range", (2, [0, 1], [0, 3], [other, other], st, w, h)),
            ("plane -2 out of range", (2, [0, 1], [-2, 1], [other, other], st, w, h)),
            ("plane 0 named twice", (2, [0, 1], [0, 0], [other, other], st, w, h)),
            ("stride %d < 3" % (3 * w - 1), (2, [0, 1], [0, 1], [other, other], [3 * w, 3 * w - 1], w, h)),
            ("does not halve to it", (2, [0, 1], [0, 1], [big, big], [big.strides[0]] * 2, 2 * w + 3, 2 * h + 1)),
            ("does not halve to it", (2, [0, 1], [0, 1], [other, other], st, w - 1, h)),
            ("does not halve to it", (2, [0, 1], [0, 1], [other, other], st, 0, 0)),
        ]
        for msg, args in uploads:
            rc_, err = _raw_upload(c, *args)
            assert rc_ != 0 and msg in err and err.startswith(("colour:", "slot")), (msg, err)
            assert good() == first, msg
        clouds = [
            ("plane -1 out of range", [(0, 1, -1, None)]),
            ("plane 3 out of range", [(0, 1, 3, None)]),
            ("plane 1 has not been written", [(0, 1, 1, None)]),
            ("slot 7 out of range", [(0, 7, 0, None)]),
            ("> max_jobs", [(0, 1, 0, None)] * 3),
        ]
        for msg, jobs in clouds:
            with pytest.raises(RuntimeError, match=msg):
                c.dense_cloud_bgr(jobs, cam, svs.IDENT, BASELINE, num_disparities=nd, block_size=bs)
            assert good() == first, msg
        # null planes / out_bgr of the cloud call
        job = (svs.DenseJob * 1)(svs.DenseJob(0, 1, 0, 0, (C.c_double * 7)(0, 0, 0, 1, 0, 0, 0)))
        prm = c._bm_params(num_disparities=nd, block_size=bs)
        xyz = np.zeros((w * h, 3), np.float32); pix = np.zeros(w * h, np.int32); bgr = np.zeros((w * h, 3), np.uint8)
        d = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(C.c_void_p)
        for planes, out in ((None, bgr.ctypes.data_as(C.c_void_p)), ((C.c_int * 1)(0), None)):
            rc_ = c.L.svslam_dense_cloud_bgr_batch(c.h, 1, job, d(cam), d(svs.IDENT), C.c_double(BASELINE), C.byref(prm), C.c_double(1.0), w * h, planes,
                                                   xyz.ctypes.data_as(C.c_void_p), pix.ctypes.data_as(C.c_void_p), out, None)
            assert rc_ != 0 and "null planes / out_bgr" in c.L.svslam_last_error(c.h).decode()
            assert good() == first
        with pytest.raises(RuntimeError, match="plane 3 out of range"):
            c.colour_read(3)
        with pytest.raises(RuntimeError, match="planes out of"):
            c.colour_reserve(-1)
        assert good() == first
        # no planes reserved: naming a plane, the cloud call and the read are refused; an upload that keeps no colour is not
        c.colour_reserve(0)
        for call in (lambda: c.pyramid_bgr([2, 3], [0, -1], [l, r]), lambda: c.colour_read(0),
                     lambda: c.dense_cloud_bgr([(0, 1, 0, None)], cam, svs.IDENT, BASELINE, num_disparities=nd, block_size=bs)):
            with pytest.raises(RuntimeError, match="no planes reserved"):
                call()
        c.pyramid_bgr([2, 3], [-1, -1], [l, r])
        c.colour_reserve(1)
        c.pyramid_bgr([2, 3], [0, -1], [l, r])
        (x, p, b, dd), = c.dense_cloud_bgr([(2, 3, 0, None)], cam, svs.IDENT, BASELINE, num_disparities=nd, block_size=bs)
        assert (x.tobytes(), p.tobytes(), b.tobytes(), dd.tobytes()) == first[:4]
    finally:
        c.close()


@pytest.mark.gpu
def test_timing_family_colour_counts_images_and_family_6_what_it_counted(svs):
    l, r, gl, gr, pl = pair(DIRECT)
    w, h = DIRECT[1]
    nd, bs = DIRECT[3]
    cam = _kitti_cam(w, h)
    assert svs.COLOUR_FAMILIES == {"colour": 18}
    assert "colour" not in svs.FAMILIES and "colour" not in svs.KERNEL_FAMILIES and 18 not in list(svs.FAMILIES.values()) + list(svs.KERNEL_FAMILIES.values())
    c = _ctx(svs, DIRECT)
    try:
        c.colour_reserve(2)
        c.timing(True)
        c.pyramid_bgr([0, 1, 2], [0, -1, 1], [l, r, l])
        ms, launches, units = c.timing_get("colour")
        assert ms > 0 and (launches, units) == (1, 3)
        assert c.timing_get("pyramid")[1:] == (1, 3)
        assert c.timing_get("stereo_bm")[1:] == (0, 0)
        c.dense_cloud([(0, 1, None), (2, 1, None)], cam, svs.IDENT, BASELINE, num_disparities=nd, block_size=bs)
        assert c.timing_get("stereo_bm")[1:] == (1, 2)
        c.dense_cloud_bgr([(0, 1, 0, None), (2, 1, 1, None)], cam, svs.IDENT, BASELINE, num_disparities=nd, block_size=bs)
        assert c.timing_get("stereo_bm")[1:] == (2, 4)
        assert c.timing_get("colour")[1:] == (1, 3)          # the cloud call adds nothing to it
    finally:
        c.close()
