"""Cases of the LiDAR corner-feature extraction, each at the smallest shape where
its rule can go wrong, and per case a *witness*: an assertion on the
definition's own state (tests/lidar_corner_ref.py) that the case really hits its
rule. A case is (cloud, Params, CornerParams, extrinsic); ``reference(name)``
evaluates the definition once per session for the CPU and the GPU tests.

Clouds are hand-placed: ``Grid`` puts one point per range-image cell, by ring
elevation and column azimuth. Connectivity is chosen through the ranges: cells at
the same range connect (the edge angle is near pi/2), a range ratio of 1.5 does
not (the angle is near the angular step). What makes a scan point a candidate is
the corner mask: rule 3 masks every point whose two scan neighbours are both
farther than 1.41 % of its range, which is every isolated point of a coarse
image. A *seed* is therefore placed next, in arrival order, to a *partner*: the
adjacent column's cell, 0.004 rad away at 1.2 % more range, near enough to lift
rule 3 and, at that range ratio, not connected to the seed. At 256 columns the partner is also too far, for its
range difference, from the cells above and below the pair to connect to them,
as long as the column beyond it stays empty (``partners_isolated`` checks that
on the definition's edge masks). After the pair comes a
*filler*, a far cell at a third range whose distance sets the seed's curvature
and with it the walk order: the seed with the farthest filler walks first."""
import functools
import math

import numpy as np

import lidar_corner_ref as CR
import lidar_feat_ref as R
from sqrtlm import lidar_feat as LF

f32 = np.float32
BASE, FAR, FILL, PARTNER = 0.5, 0.75, 1.1, 1.012
ALL = np.ones(128, np.uint8)
GAP = 0.004  # rad between a seed and its partner


def only(*rows):
    e = np.zeros(128, np.uint8)
    e[list(rows)] = 1
    return e


class Grid:
    """Points in arrival order, one per cell. The first and last point of the
    cloud are anchors in ring 20 (kept points that claim no cell of a small
    image): they fix startOri = pi and an endOri one turn later, so column c is
    the azimuth window phi in pi + [c, c + 1) 2 pi / cols."""

    def __init__(self, rows, cols):
        self.rows, self.cols, self.pts, self.cells, self.partners = rows, cols, [], {}, []

    def _pt(self, el_deg, phi, rng):
        e = math.radians(el_deg)
        return [rng * math.cos(e) * math.cos(-phi), rng * math.cos(e) * math.sin(-phi), rng * math.sin(e)]

    def add(self, r, c, rng=BASE, frac=0.5, del_deg=0.0):
        c %= self.cols
        assert (r, c) not in self.cells, (r, c)
        self.cells[(r, c)] = rng
        phi = math.pi + (c + frac) * 2.0 * math.pi / self.cols
        self.pts.append(self._pt(float(LF.ring_elevation_deg(r)) + del_deg, phi, rng))
        return self

    def run(self, cells, rng=BASE):
        for r, c in cells:
            self.add(r, c, rng)
        return self

    def seed(self, r, c, filler, rng=BASE, side=1):
        """Partner, seed, filler, in that arrival order; the partner takes column c + side."""
        half = 0.5 * GAP * self.cols / (2.0 * math.pi)
        fs, fp = (1.0 - half, half) if side > 0 else (half, 1.0 - half)
        self.add(r, c + side, rng * PARTNER, fp)
        self.partners.append((r, (c + side) % self.cols))
        self.add(r, c, rng, fs)
        if filler is not None:
            self.add(r, filler, FILL)
        return self

    def pad(self, r, c):
        return self.add(r, c, FILL)

    def cloud(self):
        a0 = self._pt(float(LF.ring_elevation_deg(20)), 0.0, 3.0)
        a1 = self._pt(float(LF.ring_elevation_deg(20)), 2.0 * math.pi - 0.01, 3.0)
        return np.asarray([a0] + self.pts + [a1], f32)


def P_small(rows, cols, **kw):
    kw.setdefault("num_curvature_regions_flat", 1)
    kw.setdefault("num_curvature_regions_corner", 1)
    kw.setdefault("num_scan_subregions", 1)
    kw.setdefault("ring_enabled", ALL)
    return LF.Params(row_num=rows, col_num=cols, **kw)


def CP_open(**kw):
    """Every ring, no ground, every curvature passes: the seed order is the subject."""
    kw.setdefault("ring_enabled", ALL)
    kw.setdefault("sharp_curv_th", -1.0)
    kw.setdefault("ground_z_bound", -100.0)
    kw.setdefault("max_corner_less_sharp", 30)
    kw.setdefault("max_corner_sharp", 3)
    return LF.CornerParams(**kw)


# ---- witnesses' helpers -------------------------------------------------------------------------

def scan_index(ref, P, r, c):
    """The position among all scan points of cell (r, c)'s scan point."""
    st = ref["corner_state"]
    off = np.concatenate([[0], np.cumsum(st["scan_n"])])
    cols = st["scan_col"][off[r]:off[r + 1]]
    k = np.flatnonzero(cols == c % P.col_num)
    assert len(k) == 1, (r, c)
    return int(off[r] + k[0])


def reason_of(ref, P, r, c):
    return int(ref["corner_state"]["reason"][scan_index(ref, P, r, c)])


def state_of(ref, P, r, c):
    return int(ref["corner_state"]["cell_state"][r, c % P.col_num])


def occupied_as_built(ref, g):
    """Every point of the grid landed in the cell it was built for."""
    st0 = ref["corner_state"]["initial_state"]
    occ = {(int(r), int(c)) for r, c in zip(*np.nonzero(st0 != -3))}
    assert occ == set(g.cells), (sorted(occ ^ set(g.cells)))
    partners_isolated(ref, g)


def partners_isolated(ref, g):
    """No edge leaves a partner cell and none leads into one."""
    e = ref["corner_state"]["edge"]
    rows, cols = e.shape
    for r, c in g.partners:
        assert e[r, c] == 0, (r, c, int(e[r, c]))
    for r, c in zip(*np.nonzero(e)):
        for k in range(6):
            if e[r, c] >> k & 1:
                assert CR.target(k, int(r), int(c), rows, cols) not in g.partners, (r, c, k)


# ---- the cases ---------------------------------------------------------------------------------

def _diag(order_a):
    """A chain down-left (r, c), (r+1, c-1), (r+2, c-2), (r+3, c-3); every other neighbour empty."""
    g = Grid(6, 256)
    chain = [(1, 20), (2, 19), (3, 18), (4, 17)]
    if order_a:  # (1, 20) is a candidate and walks first
        g.pad(1, 140).seed(1, 20, 150).pad(1, 158)
        g.pad(2, 140).seed(2, 19, 150, side=-1).pad(2, 158)
    else:        # (1, 20) has no partner: rule 3 masks it; (2, 19) seeds
        g.pad(1, 140).add(1, 20).pad(1, 150).pad(1, 158)
        g.pad(2, 140).seed(2, 19, 150, side=-1).pad(2, 158)
    g.run(chain[2:])
    P, CP = P_small(6, 256), CP_open()

    def witness(ref):
        occupied_as_built(ref, g)
        assert state_of(ref, P, 2, 20) == -3 and state_of(ref, P, 1, 19) == -3  # only the diagonal joins them
        e = ref["corner_state"]["edge"]
        assert e[1, 20] >> 5 & 1 and not e[2, 19] & 0b001111  # down-left exists; nothing leads back up
        if order_a:
            assert [state_of(ref, P, r, c) for r, c in chain] == [1, 1, 1, 1]
            assert reason_of(ref, P, 1, 20) == CR.PICKED and reason_of(ref, P, 2, 19) == CR.PICKED
        else:
            assert [state_of(ref, P, r, c) for r, c in chain] == [0, -2, -2, -2]
            assert reason_of(ref, P, 1, 20) == CR.MASKED and reason_of(ref, P, 2, 19) == CR.UNSTABLE
    return g.cloud(), P, CP, None, witness


def _wrap():
    """Seed at (1, 0): left is (1, 255), down-left is (2, 255); (2, 0) is empty."""
    g = Grid(6, 256)
    g.pad(1, 120).seed(1, 0, 130).add(1, 255).pad(1, 140)
    g.run([(2, 255), (3, 255), (3, 0), (4, 254)])
    P, CP = P_small(6, 256), CP_open()

    def witness(ref):
        occupied_as_built(ref, g)
        assert state_of(ref, P, 2, 0) == -3
        e = ref["corner_state"]["edge"]
        assert e[1, 0] >> 2 & 1 and e[1, 0] >> 5 & 1 and e[3, 255] >> 3 & 1  # left and down-left from column 0, right from 255
        assert [state_of(ref, P, r, c) for r, c in ((1, 0), (1, 255), (2, 255), (3, 255), (3, 0), (4, 254))] == [1] * 6
    return g.cloud(), P, CP, None, witness


def _linecount():
    g = Grid(8, 256)
    # A: run of 3 seeded at the top; B: run of 3 seeded in the middle; C: run of 4 seeded at an end;
    # D: seed + left neighbour + one below (2 rows); E: the same + one more below (3 rows, the seed's
    # own row flagged through its second cell); F: seed + two below, nothing beside it (2 rows)
    g.pad(1, 200).seed(1, 10, 190).seed(1, 30, 184).seed(1, 40, 196).seed(1, 50, 206).seed(1, 60, 212).pad(1, 220)
    g.run([(2, 10), (3, 10)])                      # A
    g.add(1, 20).pad(2, 200).seed(2, 20, 190).pad(2, 220).add(3, 20)  # B (row 1's (1, 20) is masked: no partner)
    g.run([(2, 30), (3, 30), (4, 30)])             # C
    g.run([(2, 40)])                               # D ...
    g.run([(2, 50), (3, 50)])                      # E ...
    g.run([(2, 60), (3, 60)])                      # F
    # the left neighbours of D and E arrive last in row 1, after the end pad: not candidates
    g.add(1, 39).add(1, 49).pad(1, 230)
    P, CP = P_small(8, 256), CP_open()

    def witness(ref):
        occupied_as_built(ref, g)
        col = lambda c, rows: [state_of(ref, P, r, c) for r in rows]
        assert col(10, (1, 2, 3)) == [-2] * 3 and col(20, (1, 2, 3)) == [-2] * 3  # 3 rows spanned, 2 flagged
        assert len(set(col(30, (1, 2, 3, 4)))) == 1 and col(30, (1,))[0] >= 1       # exactly 3 flagged
        assert col(40, (1, 2)) == [-2, -2] and state_of(ref, P, 1, 39) == -2
        assert col(50, (1, 2, 3))[0] >= 1 and state_of(ref, P, 1, 49) == col(50, (1,))[0]
        assert col(60, (1, 2, 3)) == [-2] * 3
    return g.cloud(), P, CP, None, witness


def _candidate_states():
    g = Grid(8, 256)
    # A (col 10): run of 4 with candidates in rows 1 and 3: the second is already labelled
    # B (col 30): run of 3 with candidates in rows 1 and 3: the second was set -2 by the first's growth
    # C (col 50): run rows 1..4, ground below (rows 5, 6 at z < bound), empty above: growth blocked
    # D: a ground candidate in row 6
    g.pad(1, 200).seed(1, 10, 190).seed(1, 30, 184).seed(1, 50, 196).pad(1, 220)
    g.run([(2, 10), (2, 30), (2, 50)])
    g.pad(3, 200).seed(3, 10, 190).seed(3, 30, 184).add(3, 50).pad(3, 220)
    g.run([(4, 10), (4, 50), (5, 50), (6, 50)])
    g.pad(6, 200).seed(6, 70, 190).pad(6, 220)
    z5 = BASE * math.sin(math.radians(float(LF.ring_elevation_deg(5))))  # ring 5 and below are ground
    P, CP = P_small(8, 256), CP_open(ground_z_bound=z5 * 1.2)

    def witness(ref):
        occupied_as_built(ref, g)
        s = lambda r, c: state_of(ref, P, r, c)
        assert s(1, 10) == s(3, 10) == s(4, 10) >= 1
        # 3 seeds in row 1, their 3 partners, the 2 partners of row 3: the two candidates of row 3 did not grow
        assert reason_of(ref, P, 3, 10) == CR.PICKED and ref["stats"]["seeds_grown"] == 8
        lab = ref["less_sharp_label"][[tuple(rc) == (3, 10) for rc in ref["less_sharp_rc"]]]
        assert list(lab) == [s(1, 10)]
        assert s(1, 30) == s(2, 30) == s(3, 30) == -2 and reason_of(ref, P, 3, 30) == CR.UNSTABLE
        assert s(5, 50) == -1 and s(6, 50) == -1 and s(0, 50) == -3 and s(4, 50) == s(1, 50) >= 1
        assert reason_of(ref, P, 6, 70) == CR.GROUND and s(6, 70) == -1
    return g.cloud(), P, CP, None, witness


def _caps(less, sharp):
    """Five feasible runs of 4 rows seeded in row 1, one subregion; walk order = columns 10, 20, 30, 40, 50."""
    g = Grid(6, 256)
    g.pad(1, 200)
    for k, c in enumerate((10, 20, 30, 40, 50)):
        g.seed(1, c, c + 120 - 18 * k)
    g.pad(1, 250)
    for c in (10, 20, 30, 40, 50):
        g.run([(2, c), (3, c), (4, c)])
    P, CP = P_small(6, 256), CP_open(max_corner_less_sharp=less, max_corner_sharp=sharp)

    def witness(ref):
        occupied_as_built(ref, g)
        rc = [tuple(x) for x in ref["less_sharp_rc"]]
        want = [(1, c) for c in (10, 20, 30, 40, 50)][:less]
        assert rc == want, rc
        assert len(ref["sharp_xyz"]) == min(less, sharp)
        grown = max(less, 1)  # with a cap of 0 the first candidate to reach the cap test has grown
        for k, c in enumerate((10, 20, 30, 40, 50)):
            assert (state_of(ref, P, 3, c) >= 1) == (k < grown), (k, c)
            if k >= grown:  # skipped: never grown, its cells still 0
                assert state_of(ref, P, 1, c) == 0 and reason_of(ref, P, 1, c) == CR.OVER_CAP
        if less < 5:
            assert ref["stats"]["ungrown_passing"] >= 5 - grown
        if less == 0:
            assert reason_of(ref, P, 1, 10) == CR.OVER_CAP and state_of(ref, P, 1, 10) == 1
    return g.cloud(), P, CP, None, witness


def _mask_rules(ncr_flat, ncr_corner):
    """Row 1: a seed without a partner (rule 3 alone masks it), and a pair A, B with a depth jump
    0.05 rad apart: rule 2 fires at A, masks B and its `continue` keeps rule 3 from masking A.
    Row 2: the mirrored pair, rule 1. Runs below A and the lone seed make them seeds if unmasked."""
    g = Grid(6, 256)
    w = 2 * max(ncr_flat, ncr_corner) + 2
    for r, far_first in ((1, False), (2, True)):
        for k in range(w):
            g.pad(r, 190 + 5 * k)
        g.add(r, 30)                                   # the lone seed
        g.pad(r, 60)
        if far_first:
            g.add(r, 9, FILL, 0.9).add(r, 10, BASE, 0.1)   # B then A: A is closer, rule 1 at B masks [B - c, B]
        else:
            g.add(r, 10, BASE, 0.9).add(r, 11, FILL, 0.1)  # A then B
        for k in range(w):
            g.pad(r, 120 + 5 * k)
    g.run([(3, 10), (4, 10), (5, 10), (3, 30), (4, 30), (5, 30)])
    P = P_small(6, 256, num_curvature_regions_flat=ncr_flat, num_curvature_regions_corner=ncr_corner)
    CP = CP_open()

    def witness(ref):
        occupied_as_built(ref, g)
        _, _, _, _, scans = R.image_of(g.cloud(), P)
        st = ref["corner_state"]
        off = np.concatenate([[0], np.cumsum(st["scan_n"])])
        c = ncr_corner
        for r in (1, 2):
            mask, rules, third = CR.corner_mask(scans[r], c)
            assert np.array_equal(mask, st["mask"][off[r]:off[r + 1]])
            lone = scan_index(ref, P, r, 30) - off[r]
            assert rules[lone - c] == 0 and third[lone - c] and mask[lone] == 1   # rule 3 alone
            a = scan_index(ref, P, r, 10) - off[r]
            if r == 1:
                assert rules[a - c] == 2 and mask[a] == 0 and mask[a + 1] == 1    # suppressed by rule 2's continue
                assert reason_of(ref, P, 1, 10) in (CR.PICKED, CR.UNSTABLE)
            else:
                assert rules[a - 1 - c] == 1 and mask[a - 1] == 1                # rule 1 at B
        assert ncr_flat != ncr_corner or ncr_flat == 1
    return g.cloud(), P, CP, None, witness


def _ring_range():
    g = Grid(8, 256)
    for r in (1, 2, 4, 5):
        g.pad(r, 200).seed(r, 10 + 10 * r, 180).pad(r, 220)
    P = P_small(8, 256)
    CP = CP_open(ring_enabled=None, lower_ring_num_sharp_point=3, upper_ring_num_sharp_point=5)

    def witness(ref):
        occupied_as_built(ref, g)
        assert list(np.flatnonzero(CP.enabled())) == [2, 3, 4]
        assert reason_of(ref, P, 1, 20) == CR.NONE and reason_of(ref, P, 5, 60) == CR.NONE
        assert reason_of(ref, P, 2, 30) == CR.UNSTABLE and reason_of(ref, P, 4, 50) == CR.UNSTABLE
    return g.cloud(), P, CP, None, witness


def _equal_curvatures():
    """Exactly regular lines (tests/lidar_feat_cases.lines): every corner curvature is exactly 0."""
    import lidar_feat_cases as FC
    cloud = FC.lines(40, step=3.0 / 64)
    P = LF.Params(row_num=8, col_num=1024, num_scan_subregions=1, ring_enabled=ALL)
    CP = CP_open(ring_enabled=only(6), max_corner_less_sharp=4, max_corner_sharp=2)

    def witness(ref):
        st = ref["corner_state"]
        off = np.concatenate([[0], np.cumsum(st["scan_n"])])
        c = P.num_curvature_regions_corner
        cv = st["curvature"][off[6] + c:off[7] - c]
        assert len(cv) > 8 and not cv.any()
        srt = st["sorted"][off[6] + c:off[7] - c]
        assert np.array_equal(srt, np.arange(c, c + len(srt)))          # ties: ascending index ...
        rs = st["reason"][off[6]:off[7]]
        first = [k for k in range(len(rs) - 1, -1, -1) if rs[k] not in (CR.NONE, CR.OVER_CAP)]
        assert first and first[0] == c + len(srt) - 1                   # ... so the highest index walks first
    return cloud, P, CP, None, witness


def _wall():
    """A wall filling 6 x 256 at one range: one segment larger than the workgroup and than a level's chunk."""
    g = Grid(6, 256)
    for r in range(6):
        if r == 2:
            for c in range(256):
                if c == 101:
                    continue
                if c == 100:
                    g.seed(2, 100, None)
                else:
                    g.add(2, c)
        else:
            g.run([(r, c) for c in range(256)])
    P, CP = P_small(6, 256), CP_open(ring_enabled=only(2))

    def witness(ref):
        g.partners = []  # the partner is part of the wall here
        occupied_as_built(ref, g)
        assert ref["stats"]["largest_segment"] > 1024
        assert reason_of(ref, P, 2, 100) == CR.PICKED
    return g.cloud(), P, CP, None, witness


def _snake():
    """A one-cell-wide path of 90 cells from the seed: more than 64 BFS levels."""
    g = Grid(6, 256)
    g.pad(1, 200).seed(1, 150, 230, side=1).pad(1, 245)
    g.run([(1, c) for c in range(149, 100, -1)])       # leftwards along row 1 (masked: 2.45 % apart)
    g.run([(2, 100), (3, 99), (4, 98)])                # then down-left
    g.run([(4, c) for c in range(97, 60, -1)])         # and on along row 4
    P, CP = P_small(6, 256), CP_open()

    def witness(ref):
        occupied_as_built(ref, g)
        assert ref["stats"]["most_levels"] > 64 and state_of(ref, P, 4, 61) == state_of(ref, P, 1, 150) >= 1
    return g.cloud(), P, CP, None, witness


def _empty():
    P, CP = P_small(6, 64), CP_open()
    return np.zeros((0, 3), f32), P, CP, None, lambda ref: None


def _extrinsic():
    cloud, P, CP, _, w = _caps(3, 2)
    ext = np.array([[0.0, -1.0, 0.0, 0.11], [0.0, 0.0, -1.0, -0.27], [1.0, 0.0, 0.0, 0.05], [0.0, 0.0, 0.0, 1.0]])
    return cloud, P, CP, ext, lambda ref: None


FULL_TH = 20.0  # the shipped sharp_curv_th


def _full_size():
    cloud = LF.make_sweep(3, n_az=1800, order="azimuth", start_deg=23.0, n_poles=12)
    P, CP = LF.Params(), LF.CornerParams(sharp_curv_th=FULL_TH)

    def witness(ref):
        assert len(ref["sharp_xyz"]) > 0 and ref["stats"]["cells_unstable"] > 0 and ref["stats"]["cells_labelled"] > 0
    return cloud, P, CP, None, witness


@functools.lru_cache(maxsize=None)
def cases():
    C = {}
    C["diag_seed_upper_first"] = _diag(True)
    C["diag_seed_lower_first"] = _diag(False)
    C["column_wrap"] = _wrap()
    C["linecount"] = _linecount()
    C["candidate_states"] = _candidate_states()
    for less, sharp in ((1, 1), (2, 1), (2, 5), (3, 0), (0, 0)):
        C[f"caps_{less}_{sharp}"] = _caps(less, sharp)
    C["mask_rules"] = _mask_rules(1, 1)
    C["mask_corner_wider"] = _mask_rules(1, 2)
    C["mask_flat_wider"] = _mask_rules(3, 1)
    C["ring_range"] = _ring_range()
    C["equal_curvatures"] = _equal_curvatures()
    C["wall"] = _wall()
    C["snake"] = _snake()
    C["empty"] = _empty()
    C["extrinsic"] = _extrinsic()
    C["full_size"] = _full_size()
    return C


def names(full=True):
    return [n for n in cases() if full or n != "full_size"]


@functools.lru_cache(maxsize=None)
def reference(name):
    cloud, P, CP, ext, _ = cases()[name]
    return CR.process(cloud, P, CP, ext)


def witness(name):
    cases()[name][4](reference(name))


def batches():
    """[(Params, CornerParams, [names])]: the cases with equal parameters, the batch being a property
    of one call; "full_size" and "extrinsic" stay alone."""
    out = []
    for n, (_, P, CP, ext, _) in cases().items():
        if n in ("full_size", "extrinsic"):
            continue
        key = (repr(P), P.enabled().tobytes(), repr(CP), CP.enabled().tobytes())
        for b in out:
            if b[3] == key:
                b[2].append(n)
                break
        else:
            out.append((P, CP, [n], key))
    return [b[:3] for b in out]


OUT_KEYS = ("sharp_xyz", "less_sharp_xyz", "less_sharp_label", "less_sharp_rc")
STATE_KEYS = ("cell_state", "mask", "curvature", "sorted", "reason", "edge", "angle")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def slice_of(o, k, P):
    """Sweep k of a batched features_all result as a single-sweep corner result."""
    sl, sh = int(o["sharp_off"][k]), int(o["sharp_off"][k + 1])
    ll, lh = int(o["less_sharp_off"][k]), int(o["less_sharp_off"][k + 1])
    r = dict(sharp_xyz=o["sharp_xyz"][sl:sh], less_sharp_xyz=o["less_sharp_xyz"][ll:lh],
             less_sharp_label=o["less_sharp_label"][ll:lh], less_sharp_rc=o["less_sharp_rc"][ll:lh])
    if "corner_state" in o:
        st, so, R_ = o["corner_state"], o["state"]["scan_off"], P.row_num
        a, b = int(so[k * R_]), int(so[(k + 1) * R_])
        s = {key: st[key][a:b] for key in ("mask", "curvature", "sorted", "reason")}
        for key in ("cell_state", "edge", "angle"):
            s[key] = st[key][k * R_:(k + 1) * R_]
        r["corner_state"] = s
    return r


def differences(got, want):
    """The names of everything in which a single-sweep corner result differs from the definition's."""
    bad = [k for k in OUT_KEYS if not same(got[k], want[k])]
    if "corner_state" in got:
        g, w = got["corner_state"], want["corner_state"]
        bad += [k for k in STATE_KEYS if not same(g[k], w[k])]
    return bad
