"""Cases for the tracks tests (psx_tracks_graph*, include/popsift_hip.h): synthetic record lists over edge lists, and an
independent restatement of the rule in plain Python -- a dict-based union-find followed by sorting, not a port of the C
reference.  A case is a dict: lens (rows per view), edges ((left, right) pairs), lists (one 16-byte record array per edge).
The records carry junk in their last two words: only left and right may be read."""
import numpy as np

PAIR_U8 = np.dtype([("left", "<i4"), ("right", "<i4"), ("d1", "<i4"), ("d2", "<i4")])
MEMBER = np.dtype([("view", "<i4"), ("row", "<i4")])
TOTALS = ("tracks", "members", "components", "conflicts", "too_few_views", "joined_records")
OPTIONS = [(2, False), (2, True), (3, False), (3, True)]          # (min_views, keep_conflicts)
OPTION_IDS = ["v2", "v2_keep", "v3", "v3_keep"]


def records(lefts, rights):
    out = np.zeros(len(lefts), PAIR_U8)
    out["left"], out["right"] = lefts, rights
    out["d1"] = 0x7fffffff - np.arange(len(out))        # junk that a reader of the payload would trip over
    out["d2"] = -1 - np.arange(len(out))
    return out


def concat(lists):
    return np.concatenate(lists) if len(lists) else np.zeros(0, PAIR_U8)


def restate(lists, edges, lens, min_views=2, keep_conflicts=False):
    """the rule of the header, restated: returns the totals by name, starts, member_records, labels; None where a record
    lies outside its own edge's views"""
    off = [0]
    for n in lens:
        off.append(off[-1] + int(n))
    M = off[-1]
    rep = {}

    def find(x):
        path = []
        while rep.get(x, x) != x:
            path.append(x)
            x = rep[x]
        for p in path:
            rep[p] = x
        return x

    joined = 0
    for (a, b), recs in zip(edges, lists):
        for l, r in zip(recs["left"].tolist(), recs["right"].tolist()):
            if not (0 <= l < lens[a] and 0 <= r < lens[b]):
                return None
            ga, gb = off[a] + l, off[b] + r
            if ga == gb:
                continue
            joined += 1
            ra, rb = find(ga), find(gb)
            if ra != rb:
                rep[ra] = rb                                # any representative: the root is taken as the minimum below
    view_of = [v for v, n in enumerate(lens) for _ in range(int(n))]
    groups = {}
    for g in range(M):
        groups.setdefault(find(g), []).append(g)
    comps = sorted((sorted(m) for m in groups.values() if len(m) >= 2), key=lambda m: m[0])
    out = dict(tracks=0, members=0, components=len(comps), conflicts=0, too_few_views=0, joined_records=joined)
    starts, members, labels = [0], [], [-1] * M
    for m in comps:
        views = [view_of[g] for g in m]
        conflict = len(set(views)) < len(views)
        few = len(set(views)) < min_views
        out["conflicts"] += conflict
        out["too_few_views"] += few
        if few or (conflict and not keep_conflicts):
            continue
        for g in m:
            labels[g] = out["tracks"]
            members.append((view_of[g], g - off[view_of[g]]))
        out["tracks"] += 1
        starts.append(len(members))
    out["members"] = len(members)
    out["starts"] = np.array(starts, np.int32)
    out["member_records"] = np.array(members, MEMBER) if members else np.zeros(0, MEMBER)
    out["labels"] = np.array(labels, np.int32)
    return out


# ---- the hand-written example: 4 views, 5 edges --------------------------------------------------------------------------
# lens 3, 2, 3, 2: nodes view 0 = 0 1 2, view 1 = 3 4, view 2 = 5 6 7, view 3 = 8 9
HAND = dict(
    lens=(3, 2, 3, 2),
    edges=[(0, 1), (1, 0), (0, 1), (2, 2), (2, 3)],
    lists=[
        records([0, 1], [0, 1]),      # (0, 1): 0-3, 1-4
        records([0, 1], [0, 2]),      # (1, 0), reversed: 3-0 again, 4-2 -- rows 1 and 2 of view 0 now share node 4: a conflict
        records([0], [0]),            # (0, 1) again, a duplicate edge: 0-3 a third time
        records([0, 1], [0, 2]),      # (2, 2), a self edge: 5-5 a self-loop, 6-7 two rows of one view: a conflict
        records([0], [1]),            # (2, 3): 5-9
    ])
# components: {0, 3} (2 views), {1, 2, 4} (conflict), {5, 9} (2 views), {6, 7} (conflict, one view); node 8 alone
HAND_EXPECTED = {
    (2, False): dict(tracks=2, members=4, components=4, conflicts=2, too_few_views=1, joined_records=7,
                     starts=[0, 2, 4], member_records=[(0, 0), (1, 0), (2, 0), (3, 1)], labels=[0, -1, -1, 0, -1, 1, -1, -1, -1, 1]),
    (2, True): dict(tracks=3, members=7, components=4, conflicts=2, too_few_views=1, joined_records=7,
                    starts=[0, 2, 5, 7], member_records=[(0, 0), (1, 0), (0, 1), (0, 2), (1, 1), (2, 0), (3, 1)],
                    labels=[0, 1, 1, 0, 1, 2, -1, -1, -1, 2]),
    (3, False): dict(tracks=0, members=0, components=4, conflicts=2, too_few_views=4, joined_records=7,
                     starts=[0], member_records=[], labels=[-1] * 10),
}


def deep_chain(order):
    """70 views of 1-3 rows, one row per view linked v -> v + 1: ONE component of 70 members whose root is node 0 or near it;
    the edge list reversed or shuffled, so the links arrive against the node order and the find paths grow long"""
    rng = np.random.RandomState(7)
    lens = tuple(int(x) for x in rng.randint(1, 4, 70))
    row = [int(rng.randint(0, n)) for n in lens]
    edges = [(v, v + 1) for v in range(69)]
    lists = [records([row[v]], [row[v + 1]]) for v in range(69)]
    idx = list(range(69))[::-1] if order == "reversed" else [int(i) for i in np.random.RandomState(11).permutation(69)]
    return dict(lens=lens, edges=[edges[i] for i in idx], lists=[lists[i] for i in idx])


def contention():
    """3 views x 300 rows, every row joined to row 0 of view 0: hundreds of compare-and-swaps on one root; one conflict
    component of 900 members, which crosses the 256- and 512-element workgroup boundaries of the node kernels"""
    lens = (300, 300, 300)
    rows = np.arange(300)
    return dict(lens=lens, edges=[(0, 0), (1, 0), (0, 2)],
                lists=[records(rows, np.zeros(300, np.int64)), records(rows, np.zeros(300, np.int64)), records(np.zeros(300, np.int64), rows)])


def contention_last():
    """the same with every row joined to the LAST node, row 299 of view 2: the root every lane finds keeps moving down, so
    many lanes swap on the same slot and all but one find again"""
    rows, last = np.arange(300), np.full(300, 299, np.int64)
    return dict(lens=(300, 300, 300), edges=[(0, 2), (2, 1), (2, 2)], lists=[records(rows, last), records(last, rows), records(rows, last)])


BLOCK_LENS = (0, 1, 63, 64, 65, 257, 64)
BLOCK_EDGES = [(5, 4), (2, 3), (0, 3), (3, 4), (1, 2), (4, 5), (5, 5), (2, 4), (5, 6)]
BLOCK_COUNTS = [513, 255, 0, 256, 1, 257, 64, 0, 64]


def block_edges():
    """per-edge counts of 0, 1, 255, 256, 257 and 513 records over views of 0, 1, 63, 64, 65, 257 and 64 rows; an edge with an
    empty side and count 0.  The rows walk their views with coprime strides, so the lists hold repeats, clean pairs and
    conflicts alike."""
    lists = []
    for k, ((a, b), c) in enumerate(zip(BLOCK_EDGES, BLOCK_COUNTS)):
        i = np.arange(c)
        la, lb = max(BLOCK_LENS[a], 1), max(BLOCK_LENS[b], 1)
        if (a, b) == (5, 5):
            lists.append(records(200 + i % 57, 200 + (i * (i % 9 != 0)) % 57))      # self-loops, and a same-view join at every 9th
        elif (a, b) == (5, 6):
            lists.append(records(100 + i, i))                                        # clean pairs: rows that nothing else touches ...
        elif (a, b) == (5, 4):
            lists.append(records(i % 90, (i * 3 + k) % lb))                          # rows 0 .. 89 of view 5, repeats
        elif (a, b) == (4, 5):
            lists.append(records((i * 2) % la, i % 90))
        else:
            lists.append(records((i * 5 + k) % la, (i * 3 + 1) % lb))
    return dict(lens=BLOCK_LENS, edges=list(BLOCK_EDGES), lists=lists)


def duplicate_reversed_self():
    """a duplicate edge, (a, b) beside (b, a), a left == right edge with self-loops and one genuine same-view join"""
    lens = (40, 37, 41)
    i = np.arange(30)
    return dict(lens=lens, edges=[(0, 1), (1, 0), (0, 1), (1, 2), (2, 2), (2, 1)],
                lists=[records(i, i), records(i[:20], i[:20]), records(i, i), records((i + 5) % 37, i + 3),
                       records([4, 9, 12, 40], [4, 9, 13, 40]), records(i + 3, (i + 5) % 37)])


def scattered(seed=3):
    """12 views of 0-130 rows, 40 edges in random order with random one-to-one lists: mostly clean multi-view tracks"""
    rng = np.random.RandomState(seed)
    lens = tuple(int(x) for x in rng.randint(0, 131, 12))
    edges, lists = [], []
    for _ in range(40):
        a, b = (int(x) for x in rng.randint(0, 12, 2))
        n = min(lens[a], lens[b])
        c = int(rng.randint(0, n + 1)) if n else 0
        # mostly the identity on the rows (one scene point = one row number), a few strays
        rows = rng.permutation(n)[:c]
        right = rows.copy()
        stray = rng.rand(c) < 0.03
        right[stray] = rng.randint(0, max(lens[b], 1), int(stray.sum()))
        edges.append((a, b))
        lists.append(records(rows, right))
    return dict(lens=lens, edges=edges, lists=lists)


CASES = {
    "hand": lambda: HAND,
    "chain_reversed": lambda: deep_chain("reversed"),
    "chain_shuffled": lambda: deep_chain("shuffled"),
    "contention": contention,
    "contention_last": contention_last,
    "block_edges": block_edges,
    "dup_rev_self": duplicate_reversed_self,
    "scattered": scattered,
}


def same(got, want):
    """a capi tracks dict against another (or the restatement), as bytes; returns the name of the first difference or None"""
    for k in TOTALS:
        if int(got[k]) != int(want[k]):
            return "%s %d != %d" % (k, got[k], want[k])
    for k in ("starts", "member_records", "labels"):
        if k in got and k in want and np.asarray(got[k]).tobytes() != np.asarray(want[k]).tobytes():
            return k
    return None


def raw_call(capi, fn, case, opts, track_capacity, member_capacity, with_labels=True, pairs_ptr=None, slack=3):
    """One call of a host entry point (fn takes the arguments behind `device`) on sentinel-filled arrays that are `slack`
    entries longer than the capacities: (rc, info as bytes, labels, starts, members as int32 words).  A capacity of None
    passes NULL with capacity 0."""
    import ctypes as C
    pairs = concat(case["lists"])
    ec = np.array([len(p) for p in case["lists"]], np.int32)
    ea = np.array(case["edges"], np.int32).reshape(-1, 2)
    la = np.array(case["lens"], np.int32)
    M = int(la.sum())
    labels = np.full(M + slack, -7, np.int32)
    starts = np.full((track_capacity or 0) + 1 + slack, -7, np.int32)
    members = np.full(2 * ((member_capacity or 0) + slack), -7, np.int32)
    info = capi.TracksInfo(-77, -77, -77, -77, -77, -77)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    rc = fn(ptr(pairs) if pairs_ptr is None else pairs_ptr, ptr(ec), ptr(ea), len(ea), ptr(la), len(la), C.byref(opts),
            ptr(labels) if with_labels else None, ptr(starts) if track_capacity is not None else None, track_capacity or 0,
            ptr(members) if member_capacity is not None else None, member_capacity or 0, C.byref(info))
    return rc, bytes(info), labels, starts, members
