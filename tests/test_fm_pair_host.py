"""The two host-only pieces of paired-end mapping (debwt_fm_pair_select, debwt_fm_insert_bounds), driven without a GPU
against the definitions of include/debwt_hip.h written out literally in Python."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def api():
    from debwt_amd import api as A
    return A


# a candidate: (score, record, strand, tbeg, tend)
def disjoint(a, b):
    return a[4] <= b[3] or a[3] >= b[4]


def proper(a, b, thr, lo, hi):
    """T of the proper pair (a, b) and the forward mate's tbeg, or None"""
    if a[0] < thr or b[0] < thr or a[1] != b[1] or a[2] == b[2]:
        return None
    f, r = (a, b) if a[2] == 0 else (b, a)
    if not (f[3] <= r[3] and f[4] <= r[4]):
        return None
    T = r[4] - f[3]
    return (T, f[3]) if lo <= T <= hi else None


def select_ref(c1, c2, lo, hi, penalty, min_score, seen=None):
    """debwt_fm_pair_select, clause by clause; seen (a set) collects the tie clauses that decided something"""
    seen = set() if seen is None else seen
    thr = max(1, min_score)

    def single(c):
        el = [k for k in range(len(c)) if c[k][0] >= thr]
        if not el:
            return -1
        el.sort(key=lambda k: (-c[k][0], c[k][2], c[k][1], c[k][3], k))
        if len(el) > 1 and c[el[0]][0] == c[el[1]][0]:
            a, b = c[el[0]], c[el[1]]
            seen.add("single:index" if (a[2], a[1], a[3]) == (b[2], b[1], b[3]) else "single:position")
        return el[0]

    def sub(c, w):
        if w < 0:
            return 0
        return max([c[k][0] for k in range(len(c)) if k != w and c[k][0] > 0 and disjoint(c[k], c[w])], default=0)

    b1, b2 = single(c1), single(c2)
    pp = []
    for i in range(len(c1)):
        for j in range(len(c2)):
            x = proper(c1[i], c2[j], thr, lo, hi)
            if x:
                pp.append((-(c1[i][0] + c2[j][0]), c1[i][1], x[1], i, j, x[0]))
    pp.sort()
    if len(pp) > 1 and pp[0][0] == pp[1][0]:
        seen.add("pair:index" if pp[0][1:3] == pp[1][1:3] else "pair:position")
    out = dict(i1=b1, i2=b2, proper=0, tlen=0, pair_score=0, pair_sub=0)
    if pp and -pp[0][0] >= c1[b1][0] + c2[b2][0] - penalty:
        _, _, _, i, j, T = pp[0]
        if -pp[0][0] == c1[b1][0] + c2[b2][0] - penalty:
            seen.add("choice:boundary")
        if (i, j) != (b1, b2):
            seen.add("choice:not-the-singles")
        psub = max([-p[0] for p in pp if disjoint(c1[p[3]], c1[i]) or disjoint(c2[p[4]], c2[j])], default=0)
        if psub:
            seen.add("pair_sub")
        out = dict(i1=i, i2=j, proper=1, tlen=T, pair_score=-pp[0][0], pair_sub=psub)
    elif pp:
        seen.add("choice:refused")
    out["sub1"], out["sub2"] = sub(c1, out["i1"]), sub(c2, out["i2"])
    for x, c in ((1, c1), (2, c2)):
        w = out[f"i{x}"]
        q = 0
        if w >= 0:
            s = c[w][0]
            q = 60 * (s - out[f"sub{x}"]) // s                 # negative only under a proper pair, whose term then wins
        if out["proper"]:
            P = out["pair_score"]
            q = max(q, 60 * (P - out["pair_sub"]) // P)
        out[f"mapq{x}"] = max(q, 0)
    return out


def test_pair_select_random_against_the_definition(api):
    rng = np.random.default_rng(2024)
    seen = set()
    nproper = 0
    for case in range(2000):
        cs = []
        for _ in range(2):
            c = []
            for _ in range(int(rng.integers(0, 7))):
                tb = int(rng.integers(0, 3000))
                c.append((int(rng.choice([1, 20, 29, 30, 60, 100, 100, 100, 150, int(rng.integers(1, 151))])),
                          int(rng.integers(0, 2)), int(rng.integers(0, 2)), tb, tb + int(rng.integers(1, 200))))
            if c and rng.random() < 0.3:                   # an exact copy: only the index tells them apart
                c.append(c[int(rng.integers(0, len(c)))])
            cs.append(c)
        lo = int(rng.integers(0, 400))
        hi = lo + int(rng.integers(0, 3000))
        pen = int(rng.choice([0, 17, 17, 40, 100]))
        ms = int(rng.choice([-5, 0, 30, 30, 30, 100]))
        want = select_ref(cs[0], cs[1], lo, hi, pen, ms, seen)
        got = api.pair_select(cs[0], cs[1], lo, hi, unpaired_penalty=pen, min_score=ms)
        assert got == want, (case, cs, lo, hi, pen, ms)
        nproper += want["proper"]
    assert nproper > 100
    assert seen >= {"single:index", "single:position", "pair:index", "pair:position", "choice:boundary",
                    "choice:not-the-singles", "choice:refused", "pair_sub"}, seen


F1 = (100, 0, 0, 1000, 1100)          # mate 1 forward at 1000
R2 = (100, 0, 1, 1200, 1300)          # mate 2 reverse, T = 300


def test_penalty_boundary(api):
    # mate 1 has a better single (120) elsewhere: P = 200, b1 + b2 = 220; the pair is chosen iff penalty >= 20
    c1 = [F1, (120, 1, 0, 100, 200)]
    got = api.pair_select(c1, [R2], 200, 500, unpaired_penalty=20)
    assert (got["proper"], got["i1"], got["i2"], got["tlen"], got["pair_score"]) == (1, 0, 0, 300, 200)
    assert got["sub1"] == 120 and got["mapq1"] == 60 and got["mapq2"] == 60      # the pair's term: no second pair
    got = api.pair_select(c1, [R2], 200, 500, unpaired_penalty=19)
    assert (got["proper"], got["i1"], got["i2"], got["tlen"], got["pair_score"], got["pair_sub"]) == (0, 1, 0, 0, 0, 0)
    assert got["sub1"] == 100 and got["mapq1"] == 60 * 20 // 120 and got["mapq2"] == 60


def test_geometry_and_insert_bounds(api):
    sel = lambda a, b, lo, hi: api.pair_select([a], [b], lo, hi)["proper"]
    assert sel(F1, R2, 300, 300) == 1                                         # T = ins_lo = ins_hi
    assert sel(F1, R2, 301, 500) == 0 and sel(F1, R2, 100, 299) == 0          # one outside each
    assert sel(F1, R2, 100, 300) == 1 and sel(F1, R2, 300, 900) == 1
    # reverse before forward: the same two intervals with the strands exchanged
    assert sel((100, 0, 1, 1000, 1100), (100, 0, 0, 1200, 1300), 0, 5000) == 0
    # forward contained past the reverse's end
    assert sel((100, 0, 0, 1000, 1400), (100, 0, 1, 1200, 1300), 0, 5000) == 0
    assert sel(F1, (100, 1, 1, 1200, 1300), 0, 5000) == 0                     # another record
    assert sel(F1, (100, 0, 0, 1200, 1300), 0, 5000) == 0                     # the same strand
    assert sel(R2, F1, 200, 500) == 1                                         # mate 1 may be the reverse one


def test_a_mate_without_an_eligible_candidate(api):
    got = api.pair_select([F1], [(29, 0, 1, 1200, 1300)], 200, 500)
    assert (got["i1"], got["i2"], got["proper"], got["mapq1"], got["mapq2"], got["sub2"]) == (0, -1, 0, 60, 0, 0)
    got = api.pair_select([], [], 200, 500)
    assert (got["i1"], got["i2"], got["proper"]) == (-1, -1, 0)
    # an ineligible candidate still counts for sub: the rule of debwt_fm_map
    got = api.pair_select([F1, (25, 0, 0, 2000, 2100)], [], 200, 500)
    assert (got["i1"], got["sub1"], got["mapq1"]) == (0, 25, 45)
    got = api.pair_select([(29, 0, 0, 0, 100)], [(29, 0, 1, 200, 300)], 200, 500, min_score=29)
    assert got["proper"] == 1


def test_pair_sub_from_overlapping_and_disjoint_alternatives(api):
    # a second pair whose mates both intersect the chosen ones does not count
    c1 = [F1, (90, 0, 0, 1010, 1110)]
    c2 = [R2, (90, 0, 1, 1210, 1310)]
    got = api.pair_select(c1, c2, 200, 500)
    assert (got["i1"], got["i2"], got["pair_score"], got["pair_sub"], got["mapq1"], got["mapq2"]) == (0, 0, 200, 0, 60, 60)
    # a second pair elsewhere does: mate 1's interval is disjoint (mate 2's need not be)
    c1 = [F1, (80, 0, 0, 900, 1000)]
    got = api.pair_select(c1, [R2], 200, 500)
    assert (got["pair_score"], got["pair_sub"]) == (200, 180)
    assert got["sub1"] == 80 and got["mapq1"] == max(60 * 20 // 100, 60 * 20 // 200) and got["mapq2"] == 60
    # ties of the best pair: the smaller record, then the smaller forward tbeg
    c1 = [(100, 1, 0, 5000, 5100), F1, (100, 0, 0, 990, 1090)]
    c2 = [(100, 1, 1, 5200, 5300), R2]
    got = api.pair_select(c1, c2, 200, 500)
    assert (got["i1"], got["i2"], got["tlen"]) == (2, 1, 310)


def test_pair_select_errors(api):
    with pytest.raises(api.DebwtError) as e:
        api.pair_select([F1], [R2], 500, 200)
    assert e.value.code == -1
    with pytest.raises(api.DebwtError) as e:
        api.pair_select([(10, 0, 0, 100, 100)], [R2], 200, 500)
    assert e.value.code == -1
    assert api.pair_select([(0, 0, 0, 0, 0)], [R2], 200, 500)["i1"] == -1     # score 0 with an empty interval is a non-alignment


def bounds_ref(t):
    s = sorted(int(x) for x in t)
    n = len(s)
    q1, q3 = s[n // 4], s[3 * n // 4]
    d = q3 - q1
    return max(1, q1 - 3 * d), min(16384, q3 + 3 * d)


def test_insert_bounds(api):
    rng = np.random.default_rng(5)
    with pytest.raises(api.DebwtError) as e:
        api.insert_bounds(rng.integers(250, 350, 31))
    assert e.value.code == -1
    with pytest.raises(api.DebwtError):
        api.insert_bounds([])
    for n in (32, 33, 34, 35, int(rng.integers(36, 5000))):
        t = rng.integers(200, 600, n)
        assert api.insert_bounds(t) == bounds_ref(t)
    t = np.concatenate([np.full(16, 10), np.full(16, 400)])                   # q1 - 3 d < 1
    assert api.insert_bounds(t) == bounds_ref(t) == (1, 1570)
    t = np.concatenate([np.full(16, 3000), np.full(16, 9000)])                # q3 + 3 d > 16384
    assert api.insert_bounds(t) == bounds_ref(t) == (1, 16384)
    t = np.concatenate([np.full(20, 20000), np.full(20, 20001)])
    assert api.insert_bounds(t) == bounds_ref(t) == (19997, 16384)
    assert api.insert_bounds(np.full(40, 311)) == (311, 311)                  # all equal
