"""A plain numpy restatement of the link proposal (nm_link_votes_*_u8, nm_link_rank_*) and the cases its tests share. It
does not call the library.

Votes: per ordered pair (a, b) the int64 distance matrix of the clipped frames, each row's (min1, min2) by sorting (min2 =
2139095040 for a frame of one row), and the matcher's last step: a row counts when min2 > 0 and float32(min1) / float32(min2)
< float32(ambiguity). Ranking: a Python sort on (-score, a, b) and the greedy walk.
"""
import numpy as np

MIN2_INIT = np.float32(2139095040.0)
MAX_FRAMES, MAX_LINKS = 64, 256
COUNTS = (0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257)     # the tile of 32, the wave's 64 queries, the workgroup's 256
CAPS = (1, 31, 33, 255, 257, 300)
AMBS = (0.6, 0.8, 1.0)


def clip(v, cap):
    return min(max(int(v), 0), cap)


def distances(A, B):
    """(len(A), len(B)) int64: exact squared distances of uint8 rows."""
    a, b = A.astype(np.int64), B.astype(np.int64)
    return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)


def pair_votes(A, nA, B, nB, amb):
    if nA <= 0 or nB <= 0:
        return 0
    D = np.sort(distances(A[:nA], B[:nB]), axis=1)
    min1 = D[:, 0].astype(np.float32)
    min2 = D[:, 1].astype(np.float32) if nB > 1 else np.full(nA, MIN2_INIT, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = min1 / min2
    return int(((min2 > 0) & (q < np.float32(amb))).sum())


def votes(descs, counts, cap, amb):
    n = len(descs)
    out = np.zeros((n, n), np.int32)
    for a in range(n):
        for b in range(n):
            if a != b:
                out[a, b] = pair_votes(descs[a], clip(counts[a], cap), descs[b], clip(counts[b], cap), amb)
    return out


def scores(v):
    """{(a, b): score} for a < b."""
    n = v.shape[0]
    return {(a, b): int(min(v[a, b], v[b, a])) for a in range(n) for b in range(a + 1, n)}


def rank(v, min_votes, min_gap, per_frame, max_links):
    """(link_a, link_b, link_score, count) as the entries write them: max_links entries each, -1 / -1 / 0 behind the count."""
    n = v.shape[0]
    cands = sorted((-s, a, b) for (a, b), s in scores(v).items() if b - a >= min_gap and s >= min_votes)
    deg, taken = [0] * n, []
    for ms, a, b in cands:
        if len(taken) >= max_links:
            break
        if per_frame > 0 and (deg[a] >= per_frame or deg[b] >= per_frame):
            continue
        deg[a] += 1
        deg[b] += 1
        taken.append((a, b, -ms))
    la, lb, ls = np.full(max_links, -1, np.int32), np.full(max_links, -1, np.int32), np.zeros(max_links, np.int32)
    for s, (a, b, sc) in enumerate(taken):
        la[s], lb[s], ls[s] = a, b, sc
    return la, lb, ls, len(taken)


# ---- frames ----
def world_frames(seed, n, cap, noise=6):
    """n frames of cap rows drawn from one world of 2 cap random rows, each view with its own noise: any two frames share
    about half of their rows, so the votes at 0.6 and 0.8 are neither 0 nor full."""
    rng = np.random.default_rng(seed)
    world = rng.integers(0, 256, (2 * cap, 128))
    out = []
    for _ in range(n):
        rows = world[rng.permutation(2 * cap)[:cap]] + rng.integers(-noise, noise + 1, (cap, 128))
        out.append(np.clip(rows, 0, 255).astype(np.uint8))
    return out


def tie_frames(seed, n, cap):
    """Rows of 0 / 255 only: every distance is a multiple of 255^2 near 64 of them, so equal minima, and min1 == min2, abound."""
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 2, (cap, 128)) * 255).astype(np.uint8) for _ in range(n)]


def size_cases():
    """For every n in {1, 2, 3, 5} and cap in CAPS: calls whose counts run through every entry of COUNTS that fits, and cap, and
    two that the clip takes back (cap + 7, -3). Each: dict(what, descs, counts, cap, amb)."""
    out = []
    for n in (1, 2, 3, 5):
        for cap in CAPS:
            vals = [c for c in COUNTS if c < cap] + [cap, cap + 7, -3]
            calls = (len(vals) + n - 1) // n
            for call in range(calls + (n >= 2)):
                counts = [vals[(call * n + k) % len(vals)] for k in range(n)]
                if call == calls:                                    # one more: a full frame beside sizes far from it
                    counts = [cap] + [vals[(3 * k + 1) % len(vals)] for k in range(1, n)]
                out.append(dict(what="n %d cap %d call %d counts %s" % (n, cap, call, counts), counts=counts, cap=cap,
                                descs=world_frames(1000 * n + 10 * cap + call, n, cap), amb=AMBS[(n + cap + call) % 3]))
    return out


def special_cases():
    """One-row candidate frames, duplicated candidate rows, a frame against its copy, two slots on one table, equal distances."""
    out = []
    X, Y, Z = world_frames(7, 3, 96)
    for amb in AMBS:
        out.append(dict(what="one-row candidate, amb %g" % amb, descs=[X, Y, Z], counts=[96, 1, 70], cap=96, amb=amb))
        twice = np.concatenate([X[:48], X[:48]])                     # rows 0 .. 47 of X meet their twin twice: min2 == 0
        out.append(dict(what="duplicated candidates, amb %g" % amb, descs=[X, twice, Y], counts=[96, 96, 96], cap=96, amb=amb))
        out.append(dict(what="a frame and its copy, amb %g" % amb, descs=[X, X.copy(), Y], counts=[96, 96, 33], cap=96, amb=amb))
        out.append(dict(what="two slots, one table, amb %g" % amb, descs=[X, Y, X], counts=[96, 80, 96], cap=96, amb=amb,
                        same=(0, 2)))
        out.append(dict(what="equal distances, amb %g" % amb, descs=tie_frames(11, 3, 130), counts=[130, 65, 97], cap=130, amb=amb))
    return out


def ragged64():
    """64 frames of cap 40 with ragged counts (an empty frame, a frame of one row, full frames, a count above cap)."""
    rng = np.random.default_rng(64)
    counts = [int(c) for c in rng.integers(0, 41, 64)]
    counts[5], counts[17], counts[33], counts[34], counts[63] = 0, 1, 40, 47, 40
    return dict(what="n 64 cap 40", descs=world_frames(64, 64, 40), counts=counts, cap=40, amb=0.8)


# ---- vote matrices for the ranking ----
def symmetric(n, entries, fill=0):
    v = np.full((n, n), fill, np.int32)
    np.fill_diagonal(v, 0)
    for (a, b), s in entries.items():
        v[a, b] = v[b, a] = s
    return v


def rank_cases():
    """dict(what, votes, min_votes, min_gap, per_frame, max_links) over the rules of the ranking."""
    out = []
    add = lambda what, v, mv=1, mg=1, pf=0, ml=8: out.append(dict(what=what, votes=v, min_votes=mv, min_gap=mg, per_frame=pf,
                                                                  max_links=ml))
    eq = symmetric(5, {(a, b): 9 for a in range(5) for b in range(a + 1, 5)})
    add("equal scores go by (a, b)", eq, ml=16)
    grid = symmetric(6, {(a, b): 10 + 3 * a + b for a in range(6) for b in range(a + 1, 6)})
    for mg in (1, 2, 6):
        add("min_gap %d" % mg, grid, mg=mg, ml=20)
    for mv in (16, 17, 18):                                          # score(1, 4) = 17: at, below, above
        add("min_votes %d around a score of 17" % mv, grid, mv=mv, ml=20)
    asym = symmetric(4, {(0, 1): 5, (1, 2): 6, (2, 3): 7})
    asym[0, 3], asym[3, 0] = 90, 2                                   # one direction alone does not make a link
    add("asymmetric votes score low", asym, mv=1)
    add("asymmetric votes below min_votes", asym, mv=3)
    star = symmetric(6, {(0, 1): 50, (0, 2): 49, (0, 3): 48, (1, 2): 30, (2, 3): 29, (4, 5): 10, (3, 4): 9, (1, 5): 8})
    for pf in (1, 2):                                                # the best three share frame 0
        add("per_frame %d, the best three share a frame" % pf, star, pf=pf)
    add("max_links cuts the list", grid, ml=4)
    add("max_links 1", grid, ml=1)
    add("the unused tail is filled", asym, ml=MAX_LINKS)
    add("all zero", np.zeros((7, 7), np.int32), ml=5)
    add("one frame", np.zeros((1, 1), np.int32), ml=3)
    rng = np.random.default_rng(6464)
    full = rng.integers(0, 6, (64, 64)).astype(np.int32)             # many equal scores
    add("64 x 64, few distinct scores", full, mv=1, ml=MAX_LINKS)
    add("64 x 64, per_frame 3, min_gap 2", full, mv=2, mg=2, pf=3, ml=MAX_LINKS)
    wide = rng.integers(0, 2000, (64, 64)).astype(np.int32)
    add("64 x 64, wide scores", wide, mv=500, mg=2, pf=0, ml=MAX_LINKS)
    add("64 x 64, every pair a candidate, per_frame 63", np.full((64, 64), 3, np.int32), pf=63, ml=MAX_LINKS)
    return out


# ---- what it is worth: a closed loop ----
LOOP = dict(frames=12, rows=200, step=40, window=120, noise=8.0, ambiguity=0.8, min_votes=20, min_gap=3)


def loop_frames(seed=2024):
    """A closed loop of 12 frames over a ring of 12 x 40 world points with seeded random u8 descriptors: frame k sees the 120
    points from 40 k on (wrapping), so frames one step apart share 80 points, two steps apart 40, three and more none; the
    other 80 rows of a frame are its own. Every view adds its own normal noise (sigma 8) before the clip to bytes, and a
    frame's rows are shuffled. Returns (descs, overlapping pairs {(a, b): shared points})."""
    L = LOOP
    rng = np.random.default_rng(seed)
    n, ring = L["frames"], L["frames"] * L["step"]
    world = rng.integers(0, 256, (ring, 128)).astype(np.float64)
    descs = []
    for k in range(n):
        seen = world[(L["step"] * k + np.arange(L["window"])) % ring]
        own = rng.integers(0, 256, (L["rows"] - L["window"], 128)).astype(np.float64)
        rows = np.concatenate([seen, own]) + rng.normal(0.0, L["noise"], (L["rows"], 128))
        descs.append(np.clip(np.rint(rows), 0, 255).astype(np.uint8)[rng.permutation(L["rows"])])
    shared = {}
    for a in range(n):
        for b in range(a + 1, n):
            steps = min(b - a, n - (b - a))
            if steps <= 2:
                shared[(a, b)] = L["window"] - L["step"] * steps
    return descs, shared
