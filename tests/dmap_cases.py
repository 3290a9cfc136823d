"""Seeded maps for the device-map kernel tests (tests/test_gpu_dmap_kernels.py), checked for the kernels' preconditions on the
CPU (tests/test_ref_dmap.py).  A case is a dict: `state` (the arrays of Context.dmap_state_read) plus what its stage needs.
Everything is generated from fixed seeds; nothing here depends on a GPU."""
import numpy as np

NF = 320                     # features per keyframe: feature loops cross one 256-thread chunk
MAX_LM = (256, 1024, 4096)
MAX_KF = (4, 11)
W, H = 16, 16                # the smallest frame a context accepts (the hooks read no image)
CAM_R = (20.0, 21.0, 8.0, 7.5)
BIG_ID = 2 ** 31 - 1


def empty_state(KW, NL, seed=0, junk=True):
    """a stream as svslam_create leaves it, except that what nobody may read (positions of free slots, pixels of unused
    features) holds junk instead of zeros: a kernel that reads it shows"""
    r = np.random.RandomState(seed)
    s = dict(kf_frame=np.full(KW, -1, np.int64), kf_id=np.zeros(KW, np.int32), kf_pose=np.zeros((KW, 7)), kf_n=np.zeros(KW, np.int32),
             f_xy=np.zeros((KW, NF, 2), np.float32), f_xyr=np.zeros((KW, NF, 2), np.float32), f_lm=np.full((KW, NF), -1, np.int32),
             f_lmr=np.full((KW, NF), -1, np.int32), f_fl=np.zeros((KW, NF), np.uint8), lm_pos=np.zeros((NL, 3)),
             lm_id=np.full(NL, -1, np.int32), lm_obs=np.zeros(NL, np.int32), lm_state=np.zeros(NL, np.uint8),
             lm_stamp=np.full(NL, -1, np.int32), next_lm_id=np.zeros(1, np.int32))
    if junk:
        s["f_xy"][:] = r.uniform(-50, 50, s["f_xy"].shape); s["f_xyr"][:] = r.uniform(-50, 50, s["f_xyr"].shape)
        s["lm_pos"][:] = r.uniform(-9, 9, s["lm_pos"].shape); s["kf_pose"][:] = r.uniform(-1, 1, s["kf_pose"].shape)
        s["kf_id"][:] = r.randint(0, 1000, KW); s["lm_obs"][:] = r.randint(0, 5, NL); s["lm_stamp"][:] = r.randint(0, 5, NL)
        s["f_fl"][:] = r.randint(0, 2, s["f_fl"].shape)
    return s


def rand_pose(r):
    q = r.normal(size=4); q /= np.linalg.norm(q)
    return np.concatenate([q, r.uniform(-2, 2, 3)])


class Builder:
    """puts keyframes, landmarks and observations into a state; keeps lm_obs = number of links, as the map does"""

    def __init__(self, KW, NL, seed):
        self.KW, self.NL, self.r = KW, NL, np.random.RandomState(seed)
        self.s = empty_state(KW, NL, seed + 1000)

    def keyframe(self, slot, kf_id, n, frame_id=None):
        s = self.s
        s["kf_frame"][slot] = 10 * kf_id + 3 if frame_id is None else frame_id
        s["kf_id"][slot] = kf_id; s["kf_n"][slot] = n; s["kf_pose"][slot] = rand_pose(self.r)
        s["f_lm"][slot, :n] = -1; s["f_lmr"][slot, :n] = -1; s["f_fl"][slot, :n] = 0
        return slot

    def landmark(self, slot, id_, state=1, stamp=0):
        s = self.s
        assert s["lm_id"][slot] < 0
        s["lm_id"][slot] = id_; s["lm_state"][slot] = state; s["lm_obs"][slot] = 0; s["lm_stamp"][slot] = stamp
        s["lm_pos"][slot] = self.r.uniform(-5, 5, 3) + [0, 0, 12]
        return slot

    def link(self, kf_slot, feat, lm_slot, right=False):
        s = self.s
        name = "f_lmr" if right else "f_lm"
        assert s[name][kf_slot, feat] < 0 and feat < s["kf_n"][kf_slot]
        s[name][kf_slot, feat] = lm_slot
        if right:
            s["f_fl"][kf_slot, feat] = 1
        s["lm_obs"][lm_slot] += 1


def neighbour_state(KW, NL, seed):
    """a plausible map for the streams beside the seeded one: two keyframes, some landmarks, links"""
    b = Builder(KW, NL, seed)
    b.keyframe(0, 4, 200); b.keyframe(KW - 1, 2, NF)
    for i in range(100):
        l = b.landmark((7 * i + 3) % NL, 50 + i, state=1)
        b.link(0, i, l); b.link(0, i, l, right=True); b.link(KW - 1, NF - 1 - i, l)
    b.s["next_lm_id"][0] = 150
    return b.s


# ------------------------------------------------------------------------------------------------------------ the gather
def window_slots(KW):
    """keyframe ids not in slot order, empty slots between: [(slot, kf_id)]"""
    if KW == 4:
        return [(3, 5), (0, 9), (2, 7)]                      # slot 1 empty
    return [(10, 2), (0, 30), (7, 11), (3, 4), (5, 25), (9, 6), (1, 8), (8, 17), (2, 3), (6, 40)]      # slot 4 empty


def vertex_counts(KW, NL):
    cap = min(NL, 2 * (NF * len(window_slots(KW)) - 37) - 128)      # every vertex needs a link of its own (gather_case)
    return sorted({n for n in (0, 1, 2, 3, 255, 256, 257, NL - 1, NL) if n <= cap})


def gather_case(KW, NL, nv, seed=1, big_ids=True):
    """nv vertices (active landmarks with an observation) whose ids are shuffled against their slots, some near 2^31 - 1;
    between them, where slots are left, landmarks of state 2 (with and without links) and active ones nobody observes;
    features with a right link only; every vertex has 1 .. 6 observations over the window."""
    b = Builder(KW, NL, seed + 17 * nv + NL + KW)
    r = b.r
    win = window_slots(KW)
    for slot, kid in win:
        b.keyframe(slot, kid, NF if slot != win[0][0] else NF - 37)
    slots = r.permutation(NL)
    ids = r.choice(2 ** 20, size=NL, replace=False).astype(np.int64)
    if big_ids:
        ids[: NL // 8] = BIG_ID - np.arange(NL // 8) * 3      # near the sign bit of a 32-bit id
        r.shuffle(ids)
    # free link positions, dealt in a shuffled order: (keyframe slot, feature, side)
    pos = [(slot, f, side) for slot, _ in win for f in range(int(b.s["kf_n"][slot])) for side in (0, 1)]
    order = r.permutation(len(pos))
    taken, in_kf = set(), set()
    cursor = [0]

    def next_pos(lm):
        """the next free position in a keyframe that does not see `lm` yet (the kernels' precondition: ONE feature of a keyframe
        names a landmark — on the left, on the right or on both sides)"""
        while True:
            i = int(order[cursor[0]])
            cursor[0] += 1
            slot, f, side = pos[i]
            if i in taken:
                continue
            taken.add(i)
            if (slot, lm) not in in_kf:
                in_kf.add((slot, lm))
                return i

    def link_at(i, lm):
        slot, f, side = pos[i]
        b.link(slot, f, lm, right=bool(side))
    for v in range(nv):
        l = b.landmark(int(slots[v]), int(ids[v]), state=1)
        spare = len(pos) - len(taken) - (nv - v) - 64          # positions left once every later vertex has had its one link
        for _ in range(1 + min(int(r.randint(0, 3)), max(spare, 0))):
            i = next_pos(l)
            link_at(i, l)
            twin = i ^ 1                                          # the other side of the same feature
            if spare > 8 and twin not in taken and r.rand() < 0.4:
                taken.add(twin)
                link_at(twin, l)
    others = [int(x) for x in slots[nv:nv + min(40, NL - nv)]]
    for k, l in enumerate(others):
        kind = k % 3
        b.landmark(l, int(ids[nv + k]), state=2 if kind < 2 else 1)
        if kind == 0 and len(taken) + 72 < len(pos):            # outside the window but carried by tracking: a link, no edge
            link_at(next_pos(l), l)
    b.s["next_lm_id"][0] = 77
    return dict(state=b.s)


def gather_cases():
    out = []
    for KW in MAX_KF:
        for NL in MAX_LM:
            for nv in vertex_counts(KW, NL):
                out.append(("kw%d-nl%d-nv%d" % (KW, NL, nv), KW, NL, nv))
    return out


def chain_case(KW=4, NL=256, seed=5):
    """a consistent three-keyframe map whose landmarks project where their features are: a local BA converges on it"""
    import ref_dmap
    b = Builder(KW, NL, seed)
    r = b.r
    cam = (350.0, 350.0, 310.0, 94.0)
    win = [(2, 1), (0, 2), (3, 3)]
    poses = {}
    for a, (slot, kid) in enumerate(win):
        b.keyframe(slot, kid, 120)
        p = np.array([0.002 * a, -0.001 * a, 0.0015 * a, 1.0, -0.3 * a, 0.01 * a, -0.05 * a]); p[:4] /= np.linalg.norm(p[:4])
        b.s["kf_pose"][slot] = p
        poses[slot] = p
    ext_r = np.array([0, 0, 0, 1, -0.54, 0, 0.0])
    for i in range(100):
        l = b.landmark(int((11 * i + 5) % NL), 900 - 7 * i)
        X = np.array([r.uniform(-6, 6), r.uniform(-2, 2), r.uniform(8, 30)])
        b.s["lm_pos"][l] = X + r.normal(scale=0.05, size=3)
        for slot, _ in win:
            if r.rand() < 0.25:
                continue
            T = poses[slot]
            Tr = T.copy(); Tr[4:] = T[4:] + ext_r[4:]          # the right camera: a pure shift along x behind the pose
            u = ref_dmap.project(T, cam, X); ur = ref_dmap.project(Tr, cam, X)
            noise = r.normal(scale=0.3, size=4)
            b.link(slot, i, l); b.link(slot, i, l, right=True)
            b.s["f_xy"][slot, i] = (u[0] + noise[0], u[1] + noise[1]); b.s["f_xyr"][slot, i] = (ur[0] + noise[2], ur[1] + noise[3])
    for l in range(NL):                                       # landmarks nobody observes would be vertices without edges
        if b.s["lm_id"][l] >= 0 and b.s["lm_obs"][l] == 0:
            b.s["lm_id"][l] = -1; b.s["lm_state"][l] = 0
    b.s["next_lm_id"][0] = 1000
    return dict(state=b.s, cam=cam, ext_l=np.array([0, 0, 0, 1, 0, 0, 0.0]), ext_r=ext_r)


# ------------------------------------------------------------------------------------------------------------ the scatter
def edges_case(KW, NL, nobs, seed=3):
    """exactly nobs edges: landmark v takes up to four links, the left and the right feature v of the first keyframe first
    (both edges of ONE feature), then a left feature of the second and a right feature of the third keyframe"""
    b = Builder(KW, NL, seed + nobs)
    win = window_slots(KW)[:3]
    for slot, kid in win:
        b.keyframe(slot, kid, NF)
    where = [(win[0][0], False), (win[0][0], True), (win[1][0], False), (win[2][0], True)]
    ids = b.r.permutation(5 * NL)[:NL] + 1
    for e in range(nobs):
        v, k = divmod(e, 4)
        l = int((37 * v + 11) % NL)
        if k == 0:
            b.landmark(l, int(ids[v]))
        b.link(where[k][0], v, l, right=where[k][1])
    b.s["next_lm_id"][0] = int(ids.max()) + 1
    return dict(state=b.s)


SCATTER_NOBS = (1, 255, 256, 257)


# ------------------------------------------------------------------------------------------------------------ begin
STAMP = 41                   # the step's stamp in the begin / commit cases; older steps stamped 0 .. 5


def begin_case(KW, NL, ncand, seed=7, npts=300):
    """a full window whose oldest keyframe retires.  Its features name landmarks on the left only, on the right only and on both
    sides; min(ncand, 3) of those landmarks have no other observer (CleanMap takes them out and they are candidates at once),
    the rest of the ncand candidates are landmarks that were outside the window already.  The tracked list has survivors with
    and without a map point, one of them a state-2 landmark nobody observes: stamped by this step, it stays."""
    b = Builder(KW, NL, seed + ncand + NL)
    r = b.r
    win = window_slots(KW)
    for slot, kid in win:
        b.keyframe(slot, kid, 280)
    free_kf = sorted(set(range(KW)) - {s for s, _ in win})[0]
    old = min(win, key=lambda t: t[1])[0]
    other = [s for s, _ in win if s != old]
    slots = [int(x) for x in r.permutation(NL)]
    ids = [int(x) for x in r.permutation(10 * NL)[:NL]]
    nshared = min(60, NL // 4)
    lone, lone_slots = min(ncand, 3), []
    for i in range(nshared):                                  # observed by the retiring keyframe and by another one
        l = b.landmark(slots.pop(), ids.pop())
        side = i % 3                                          # 0 left only, 1 right only, 2 both
        if side in (0, 2):
            b.link(old, 2 * i, l)
        if side in (1, 2):
            b.link(old, 2 * i, l, right=True)
        b.link(other[i % len(other)], i, l, right=bool(i & 1))
    for i in range(lone):                                     # observed by the retiring keyframe alone
        l = b.landmark(slots.pop(), ids.pop(), stamp=3)
        lone_slots.append(l)
        if i % 3 in (0, 2):
            b.link(old, 200 + i, l)
        if i % 3 in (1, 2):
            b.link(old, 200 + i, l, right=True)
    for i in range(ncand - lone):                             # outside the window, unobserved, not carried: candidates
        b.landmark(slots.pop(), ids.pop(), state=2, stamp=int(r.randint(0, 6)))
    carried = b.landmark(slots.pop(), ids.pop(), state=2, stamp=2)          # named by the tracked list below: kept
    b.landmark(slots.pop(), ids.pop(), state=2, stamp=STAMP)                # stamped by this step already: kept
    seen = b.landmark(slots.pop(), ids.pop(), state=2, stamp=1)             # outside the window but still observed: kept
    b.link(other[0], 270, seen)
    # the tracked survivors: map points of landmarks the window observes, the carried one, and features without one
    named = [l for l in range(NL) if b.s["lm_state"][l] == 1 and b.s["lm_obs"][l] > 0 and l not in lone_slots]
    r.shuffle(named)
    mp = np.full(npts, -1, np.int32)
    take = named[: min(len(named), npts // 2)] + [carried]
    where = r.permutation(npts)[: len(take)]
    mp[where] = take
    xy = r.uniform(0, 600, (npts, 2)).astype(np.float32)
    xyz = r.uniform(-5, 5, (npts, 3))
    job = dict(is_init=0, kf_slot=free_kf, remove_slot=old, kf_id=max(k for _, k in win) + 1, frame_id=777, npts=npts, stamp=STAMP,
               pose=rand_pose(r))
    b.s["next_lm_id"][0] = 10 * NL
    return dict(state=b.s, job=job, xy=xy, mp=mp, xyz=xyz, ncand=ncand)


def begin_quota(NL):
    return 8 if NL == 256 else 300


def begin_counts(NL):
    q = begin_quota(NL)
    return (0, 1, q - 1, q, q + 1, 3 * q)


# ------------------------------------------------------------------------------------------------------------ commit
def commit_case(KW, NL, n_tri_in, nfree, seed=11, is_init=False, npts=NF):
    """a keyframe after stereo_finish: n_tri_in pairs to triangulate (features without a map point, in feature order), a mixed
    tri_ok; nfree free landmark slots scattered through the arena, the others taken by landmarks outside the window"""
    b = Builder(KW, NL, seed + n_tri_in + nfree)
    r = b.r
    slot = 1
    if is_init:
        b.s["kf_n"][slot] = npts
        b.s["f_lm"][slot, :npts] = -1; b.s["f_lmr"][slot, :npts] = -1
    else:
        b.keyframe(slot, 12, npts)
    free = set(int(x) for x in r.permutation(NL)[:nfree])
    ids = r.permutation(8 * NL)[:NL]
    for l in range(NL):
        if l not in free:
            b.landmark(l, int(ids[l]), state=2, stamp=STAMP)
    rt = np.random.RandomState(seed * 7919 + n_tri_in)        # the triangulation's results do not depend on nfree: the accepted count
    tri_idx = np.sort(rt.permutation(npts)[:n_tri_in]).astype(np.int32)      # of a given n_tri_in is one number the free slots are set against
    tri_ok = (rt.rand(n_tri_in) < 0.7).astype(np.uint8)
    tri_xyz = rt.uniform(-20, 20, (n_tri_in, 3))
    b.s["f_fl"][slot, tri_idx] = 1
    b.s["next_lm_id"][0] = 8 * NL + 5
    job = dict(is_init=1 if is_init else 0, kf_slot=slot, remove_slot=-1, kf_id=0 if is_init else 12, frame_id=5 if is_init else 123,
               npts=0 if is_init else npts, n_features=npts, n_tri_in=n_tri_in, stamp=STAMP, dead=0, pose=rand_pose(r))
    return dict(state=b.s, job=job, tri_idx=tri_idx, tri_ok=tri_ok, tri_xyz=tri_xyz, accepted=int(tri_ok.sum()))


# ------------------------------------------------------------------------------------------------------------ prep, finish, refresh
def feature_case(KW, NL, npts, seed=13, with_mp=True):
    """a keyframe as begin leaves it: npts tracked features, every other one with a map point"""
    b = Builder(KW, NL, seed + npts)
    slot = 2
    b.keyframe(slot, 6, npts)
    b.keyframe(0, 3, 50)
    if with_mp:
        slots = b.r.permutation(NL)
        for i in range(0, min(npts, 2 * NL - 2), 2):
            l = b.landmark(int(slots[i // 2]), 400 + i)
            b.link(slot, i, l)
            if i % 4 == 0 and i // 4 < 50:
                b.link(0, i // 4, l)
    return dict(state=b.s, slot=slot)
