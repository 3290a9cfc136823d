"""A plain statement of the structure rule of a local-BA problem — which landmark gets which internal number, which go
through the LDS tiles, where a tile ends — written from the comments of BaHostStruct::build (csrc/k_ba.h: "Landmarks are
renumbered by descending block count ..." and "LDS tiles: consecutive landmarks ..."), not from its code.  numpy / plain
Python only; tests/test_ref_ba_structure.py checks it against brute force, tests/test_gpu_ba_structure.py checks
BaHostStruct::build and k_ba_build against it through Context.ba_struct.

The rule
  * a BLOCK is a (landmark, keyframe) pair with at least one edge (a left and a right edge of one keyframe share a block);
  * landmarks are renumbered by descending block count, stable in the caller's numbering;
  * GROUPED numbering (max block count >= 1 and max block count + nkf <= BB_MAXKEYS): the landmarks with one block are
    ordered by the keyframe of that block (sv_start[k] = first landmark of keyframe k's group, sv_start[nkf] = first
    landmark without edges), landmarks without edges come last, nmv = sv_start[0] = landmarks with two or more blocks;
  * UNGROUPED numbering (too many keys): descending block count only, nmv = nlm, sv_start is nlm everywhere;
  * landmarks [0, nmv) are cut into LDS tiles greedily: consecutive landmarks, at most tile_cap landmarks and at most
    tile_cap blocks per tile;
  * a landmark with m blocks lists m (m + 1) / 2 block pairs ("items") in its tile; ncontrib is their total;
  * na = keyframes with at least one edge, nblk = blocks in all.

The constants below restate csrc/k_ba.h and csrc/k_ba_build.h.  Whoever changes one of them there changes it here:
  BA_THREADS, BA_LDS_LIMIT, BA_WAVES, BA_ROWS, BA_MAX_NP, BA_PIT_CAP, BA_TILE_MAX, BB_MAXKEYS   k_ba.h:40-53
  BA_PT, BA_CT                                                                                 k_ba.h "LDS pose table entry"
  ba_lds_fixed_bytes, ba_tile_cap                                                              k_ba.h, below k_local_ba_t
  BB_THREADS, bb_lds_ints, bb_edge_cache_fits, bb_lds_bytes                                    k_ba_build.h:19, 54-64
  LL_ECAP, LL_LCAP, ba_lds_fixed_bytes_ll, ba_tile_cap_ll                                      k_ba.h (low-latency shards)
  LlCaps, ba_ll_lds_bytes, ba_ll_caps                                                          k_ba_ll.h:23-46
  the dealing rule (ll_deal)                                                                   k_ba_build.h:327-332, 386-396
  what k_ba_build does for a shard (structure(no_group, all_active))                           k_ba_build.h:150-151, 172-173
  ll_shard_in_lds                                                                              k_ba.h "const bool ll_res"
  ll_enabled, ll_tile_cap                             api_ba.h svslam_set_low_latency, svslam_hip.hip ba_ll_tile_cap
"""
import numpy as np

BA_THREADS = 512
BA_LDS_LIMIT = 160 * 1024
BA_WAVES = BA_THREADS // 64
BA_ROWS = BA_THREADS // 16
BA_MAX_NP = 192
BA_PIT_CAP = 2048
BA_TILE_MAX = 480
BB_MAXKEYS = 33
BB_THREADS = 256
BA_PT = 12
BA_CT = 16
EDGE_CACHE_LIMIT = 150 * 1024
CREATE_BUILD_LDS_LIMIT = 160 * 1024         # svslam_create: bb_lds_bytes(max_lm) must fit
LIST_CHUNK = BB_MAXKEYS * BB_THREADS        # pair lists k_ba_build emits per pass


def lds_fixed_bytes(max_kf):
    """LDS of the batch solver besides the tile: the (np + 1)^2 reduced system, 4 np vectors, 36 doubles per keyframe,
    the wave partials, two pose tables, two cameras, 32 doubles per 16-lane row; the pair ranges and BA_PIT_CAP items"""
    n = 6 * max_kf
    doubles = (n + 1) * (n + 1) + 4 * n + 36 * max_kf + BA_WAVES + 2 * BA_PT * max_kf + 2 * BA_CT + 32 * BA_ROWS
    kmax = BA_MAX_NP // 6
    ints = kmax * (kmax + 1) // 2 + 1 + BA_PIT_CAP
    return 8 * doubles + 4 * ints + 64


def tile_cap(max_kf):
    """landmarks / blocks per LDS tile: 27 doubles each in what the LDS limit leaves, a multiple of 16, at most BA_TILE_MAX;
    0 when not even 64 fit"""
    fixed = lds_fixed_bytes(max_kf)
    if fixed + 27 * 8 * 64 > BA_LDS_LIMIT:
        return 0
    t = (BA_LDS_LIMIT - fixed) // (27 * 8)
    return min(t // 16 * 16, BA_TILE_MAX)


def bb_lds_ints(max_nlm):
    """LDS ints of k_ba_build for a batch whose largest problem has max_nlm landmarks: six per-landmark arrays,
    the [key][thread] counters, a scan row, five per-key rows, scalars"""
    return 6 * (max_nlm + 2) + BB_MAXKEYS * BB_THREADS + BB_THREADS + 5 * BB_MAXKEYS + 64


def edge_cache_fits(max_nlm, max_nobs):
    """one packed word per edge of the batch's largest problem still fits beside that"""
    return 4 * (bb_lds_ints(max_nlm) + max_nobs) <= EDGE_CACHE_LIMIT


def bb_lds_bytes(max_nlm, max_nobs=0):
    return 4 * (bb_lds_ints(max_nlm) + (max_nobs if edge_cache_fits(max_nlm, max_nobs) else 0))


# ---- the low-latency solver: a problem dealt to shards, each solved by a kernel that keeps the shard in LDS when it fits
# The capacities are the LDS budgets of k_ba.h / k_ba_ll.h and the fit test of k_ba_split restated term by term
# (tests/test_ref_ba_structure.py pins their values at max_kf 7, 11, 13, 16, 17); the shard sizes they are applied to come from
# ll_deal below, which is written from the dealing rule and held to a loop-only second implementation.
LL_ECAP = 704
LL_LCAP = 448
BAREC_BYTES = 16            # BaRec: two floats, two ints


def tile_cap_ll(max_kf):
    """tile capacity of the streaming shard kernel: the batch layout, two copies of LL_ECAP records and of LL_LCAP positions,
    an int per block"""
    fixed = lds_fixed_bytes(max_kf) + 2 * LL_ECAP * BAREC_BYTES + 6 * LL_LCAP * 8 + 64
    per = 27 * 8 + 4
    if fixed + per * 64 > BA_LDS_LIMIT:
        return 0
    return min((BA_LDS_LIMIT - fixed) // per // 16 * 16, BA_TILE_MAX)


def ll_resident_lds_bytes(max_kf, B, L, E):
    n = 6 * max_kf
    doubles = ((n + 1) * (n + 1) + 5 * n + 72 * max_kf + BA_WAVES + 2 * BA_PT * max_kf + 2 * BA_CT + 14 * max_kf + 32 * BA_ROWS
               + 15 * L + 27 * B)
    kmax = BA_MAX_NP // 6
    ints = (L + 1) + 3 * (B + 1) + E + 40 + kmax * (kmax + 1) // 2 + 1 + BA_PIT_CAP + 16
    return 8 * doubles + BAREC_BYTES * E + 4 * ints + 64


def ll_caps(max_kf):
    """(blocks, landmarks, edges) of a shard the resident kernel holds: 208 landmarks, 448 edges, and the blocks the LDS
    limit leaves (a multiple of 16, at most 320); (0, 0, 0) when not even 64 blocks fit"""
    L, E = 208, 448
    fixed = ll_resident_lds_bytes(max_kf, 0, L, E)
    per = 27 * 8 + 12
    if fixed + 64 * per > BA_LDS_LIMIT:
        return 0, 0, 0
    return min((BA_LDS_LIMIT - fixed) // per // 16 * 16, 320), L, E


def ll_shards_fit(max_kf, shard_nlm, shard_nobs, shard_nblk):
    """do all shards of a problem (sizes as Context.ll_shards reports them) fit the resident kernel?  A shard has one tile
    there, of the smaller of the two kernels' capacities"""
    B, L, E = ll_caps(max_kf)
    if B <= 0:
        return False
    cap = min(tile_cap_ll(max_kf), B)
    return bool(np.all(np.asarray(shard_nblk) <= min(B, cap)) and np.all(np.asarray(shard_nlm) <= min(L, cap))
                and np.all(np.asarray(shard_nobs) <= E))


def ll_enabled(max_kf):
    """svslam_set_low_latency makes the shard solver only where the streaming kernel's tile holds a landmark seen from every
    keyframe and at least 64 blocks: tile_cap_ll(max_kf) >= max(max_kf, 64) (true up to max_kf 16)"""
    return tile_cap_ll(max_kf) >= max(max_kf, 64)


def ll_tile_cap(max_kf, resident):
    """ba_ll_tile_cap: the tile capacity the shards are built with is what BOTH shard kernels hold, min(tile_cap_ll, B) in a
    context with the resident kernel, tile_cap_ll in one without (SVSLAM_LL_RESIDENT=0: B = 0)"""
    t, B = tile_cap_ll(max_kf), ll_caps(max_kf)[0]
    return min(t, B) if resident and B > 0 else t


def ll_shard_in_lds(nlm, nobs):
    """k_local_ba_t<2>: a shard's records and positions live in LDS when it has at most LL_ECAP edges and LL_LCAP landmarks,
    decided per shard"""
    return nobs <= LL_ECAP and nlm <= LL_LCAP


def ll_deal(olm, okf, nlm, W):
    """k_ba_split's dealing rule for the edges (olm[e], okf[e]), landmark-major with keyframes ascending inside a landmark,
    over W shards.  A landmark with e edges costs e (4 + e); the shard of a landmark is floor(cost of the landmarks before it
    x W / total cost), at most W - 1; the shards are contiguous ranges in landmark order and a shard nothing fell into is the
    empty range at the next shard's first landmark (at nlm behind the last); the mask has a bit for every shard with an edge;
    a block is a distinct (landmark, keyframe) pair.  Python integers throughout.
    Returns dict(cut [W + 1], nlm [W], nobs [W], nblk [W], mask)."""
    olm = [int(v) for v in olm]; okf = [int(v) for v in okf]
    assert len(olm) == len(okf) >= 1 and all(0 <= l < nlm for l in olm)
    assert all((olm[i], okf[i]) <= (olm[i + 1], okf[i + 1]) for i in range(len(olm) - 1)), "edges are not landmark-major"
    edges = [0] * nlm
    for l in olm:
        edges[l] += 1
    cost = [e * (4 + e) for e in edges]
    before = [sum(cost[:l]) for l in range(nlm)]
    total = sum(cost)
    shard = [min(before[l] * W // total, W - 1) for l in range(nlm)]
    assert all(shard[l] <= shard[l + 1] for l in range(nlm - 1))
    cut = [None] * W + [nlm]
    for w in range(W - 1, -1, -1):
        own = [l for l in range(nlm) if shard[l] == w]
        cut[w] = own[0] if own else cut[w + 1]
    blocks = sorted(set(zip(olm, okf)))
    s_nlm = [cut[w + 1] - cut[w] for w in range(W)]
    s_nobs = [sum(edges[cut[w]:cut[w + 1]]) for w in range(W)]
    s_nblk = [sum(1 for l, _ in blocks if cut[w] <= l < cut[w + 1]) for w in range(W)]
    mask = sum(1 << w for w in range(W) if s_nobs[w] > 0)
    return dict(cut=cut, nlm=s_nlm, nobs=s_nobs, nblk=s_nblk, mask=mask)


def ll_shards(olm, okf, nkf, nlm, W, max_kf, resident):
    """what Context.ll_shards reports for the problem, one row per shard: landmarks, edges, blocks, tiles, solver code (2:
    resident k_ba_ll, 1: streaming k_local_ba_t<2>), active poses, shard mask — the deal, k_ba_build's structure of every shard
    (no_group, all_active; a shard without edges is not built: no blocks, tiles or poses), and k_ba_split's fit test.
    Also returns the per-shard structures (None for a shard without edges)."""
    olm = np.asarray(olm, np.int64); okf = np.asarray(okf, np.int64)
    d = ll_deal(olm, okf, nlm, W)
    cap = ll_tile_cap(max_kf, resident)
    fits = bool(resident) and ll_shards_fit(max_kf, d["nlm"], d["nobs"], d["nblk"])
    rows, structs = [], []
    for w in range(W):
        a, b = d["cut"][w], d["cut"][w + 1]
        sel = (olm >= a) & (olm < b)
        s = structure(nkf, b - a, okf[sel], olm[sel] - a, cap, no_group=True, all_active=True) if sel.any() else None
        assert s is None or (s["nblk"] == d["nblk"][w] and s["nlm"] == d["nlm"][w])
        structs.append(s)
        rows.append([d["nlm"][w], d["nobs"][w], d["nblk"][w], s["ntile"] if s else 0, 2 if fits else 1, s["na"] if s else 0,
                     d["mask"]])
    return np.array(rows, np.int64), structs, d


def structure(nkf, nlm, okf, olm, cap, no_group=False, all_active=False):
    """the structure of the problem with edges (okf[e], olm[e]), any order, for tiles of capacity `cap`; nobs >= 1
    (a problem without edges is not built at all).  no_group, all_active: what k_ba_build is told for a low-latency shard —
    ungrouped numbering whatever the key count (nmv = nlm: every landmark goes through the tiles, the ones without edges
    too), and every keyframe an active pose (na = nkf)"""
    okf = np.asarray(okf, np.int64); olm = np.asarray(olm, np.int64)
    assert len(okf) == len(olm) >= 1 and okf.min() >= 0 and okf.max() < nkf and olm.min() >= 0 and olm.max() < nlm
    seen = np.zeros((nlm, nkf), bool)
    seen[olm, okf] = True
    blocks = seen.sum(1)                                         # per landmark, caller numbering
    maxc = int(blocks.max())
    grouped = not no_group and maxc >= 1 and maxc + nkf <= BB_MAXKEYS
    only_kf = seen.argmax(1)                                     # meaningful where blocks == 1

    def rank(l):
        m = int(blocks[l])
        if not grouped:
            return (-m, 0)
        if m >= 2:
            return (0, -m)
        return (1, int(only_kf[l])) if m == 1 else (2, 0)
    lm_orig = np.array(sorted(range(nlm), key=rank), np.int64)   # sorted() is stable
    b = blocks[lm_orig]                                          # per landmark, internal numbering
    if grouped:
        nmv = int((b >= 2).sum())
        single_kf = only_kf[lm_orig][b == 1]
        sv_start = np.array([nmv + int((single_kf < k).sum()) for k in range(nkf + 1)], np.int64)
    else:
        nmv = nlm
        sv_start = np.full(nkf + 1, nlm, np.int64)
    tile_lm = [0]
    nl = nb = 0
    for l in range(nmv):
        if nl + 1 > cap or nb + int(b[l]) > cap:
            tile_lm.append(l); nl = nb = 0
        nl += 1; nb += int(b[l])
    if nmv > 0:
        tile_lm.append(nmv)
    tile_lm = np.array(tile_lm, np.int64)
    ntile = len(tile_lm) - 1
    items_lm = b * (b + 1) // 2
    tile_items = np.array([int(items_lm[tile_lm[t]:tile_lm[t + 1]].sum()) for t in range(ntile)], np.int64)
    tile_blocks = np.array([int(b[tile_lm[t]:tile_lm[t + 1]].sum()) for t in range(ntile)], np.int64)
    na = nkf if all_active else int(seen.any(0).sum())
    return dict(nkf=nkf, nlm=nlm, cap=cap, blocks=blocks, maxc=maxc, grouped=grouped, lm_orig=lm_orig, blocks_new=b, nmv=nmv,
                sv_start=sv_start, na=na, nblk=int(blocks.sum()), tile_lm=tile_lm, ntile=ntile, tile_items=tile_items,
                tile_blocks=tile_blocks, ncontrib=int(tile_items.sum()), npairs=na * (na + 1) // 2,
                nlists=ntile * (na * (na + 1) // 2))


def list_chunks(s):
    """passes k_ba_build needs to emit the (tile, pose pair) lists"""
    return -(-s["nlists"] // LIST_CHUNK)
