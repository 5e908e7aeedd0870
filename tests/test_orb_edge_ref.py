"""The conditions on the inputs of tests/orb_edge_cases.py, asserted on the CPU
oracle alone, so that tests/test_gpu_orb_edges.py cannot pass empty: the
cell-occupancy classes, keypoints outside the grid, a candidate list longer
than two ballots, the BoW run lengths, the mod-4 coverage of the extractor's
level widths and the match counts of every search. The thresholds are
conditions the seeds were chosen for, not measurements.

The oracle is taken to new edges here too, so it is checked against the
pure-Python transliterations (tests/orb_translit.py) on the same frames."""
import numpy as np
import pytest

import orb_edge_cases as E


@pytest.fixture(scope="module")
def OB(oracle):
    from oracle import orb as OB
    return OB


def test_crowd_frame_conditions(OB):
    F = E.crowd()
    k2 = F.k2
    assert len(k2) == len(F.k1) == 601 and len(k2) % 4 == 1
    minx, maxx, miny, maxy = F.bounds
    assert all(v != 0 and v != int(v) for v in F.bounds)
    px, py, inside = E.pos_in_grid(k2)
    occ = np.zeros((E.GRID_COLS, E.GRID_ROWS), int)
    np.add.at(occ, (px[inside], py[inside]), 1)
    got = sorted(int(occ[cx, cy]) for cx, cy, _ in E.CLUSTERS)
    assert got[0] == 64 and 65 <= got[1] <= 128 and got[2] > 128
    assert got == sorted(c[2] for c in E.CLUSTERS)
    assert occ[E.GRID_COLS - 1, E.GRID_ROWS - 1] > 128  # a crowded cell on the last column and row
    others = occ.copy()
    for cx, cy, _ in E.CLUSTERS:
        others[cx, cy] = 0
    assert others.max() < 64  # nothing else reaches a second ballot
    # outside the bounds and outside the grid on each side
    for out in (k2["x"] < minx, k2["x"] > maxx, k2["y"] < miny, k2["y"] > maxy):
        assert out.any()
    assert (px < 0).any() and (px >= E.GRID_COLS).any() and (py < 0).any() and (py >= E.GRID_ROWS).any()
    # outside the bounds, yet rounded into the first / last cell
    assert ((k2["x"] < minx) & inside).any() and ((k2["y"] < miny) & inside).any()
    assert sorted(set(k2["octave"].tolist())) == list(range(8))
    assert sorted(set(F.k1["octave"].tolist())) == list(range(8))
    # identical descriptors inside one cell
    D = E.hamming_matrix(F.d2, F.d2)
    i, j = np.nonzero(np.triu(D == 0, 1))
    assert len(i) >= 5 and (px[i] == px[j]).all() and (py[i] == py[j]).all() and inside[i].all()
    assert (k2["octave"][i] == k2["octave"][j]).all()
    # frame 1: shifted, permuted, a few bits flipped
    assert not np.array_equal(F.src, np.arange(601))
    assert np.abs(k2["x"][F.src] - F.k1["x"] - E.SHIFT[0]).max() < 1e-4  # float32 coordinates up to 660
    assert np.abs(k2["y"][F.src] - F.k1["y"] - E.SHIFT[1]).max() < 1e-4
    assert (np.unpackbits(F.d1 ^ F.d2[F.src], axis=1).sum(axis=1) == 6).all()
    assert (F.k1["angle"] != k2["angle"][F.src]).all()


def test_crowd_candidate_lists_span_three_ballots(OB):
    F = E.crowd()
    px, py, inside = E.pos_in_grid(F.k2)
    cx, cy, n = E.CLUSTERS[-1]
    members = np.nonzero((px == cx) & (py == cy))[0]
    assert len(members) == n
    c = members[0]
    got = OB.features_in_area(F.k2, F.bounds, F.k2["x"][c], F.k2["y"][c], 10.0)
    assert len(got) > 128 and set(members) <= set(got.tolist())


def test_bow_run_lengths():
    for seed in (E.seed_of("crowd"), E.seed_of("crowd") + 2):  # the BoW searches, SearchForTriangulation
        n1, n2 = E.bow_nodes("crowd", seed)
        ids, cnt = np.unique(n2[n2 >= 0], return_counts=True)
        assert sorted(cnt.tolist()) == sorted(E.BOW_RUNS)
        assert {1, 63, 64, 65, 128, 129} <= set(cnt.tolist()) and cnt.max() > 129
        assert (n2 < 0).sum() == 601 - sum(E.BOW_RUNS) > 0
        # every run is searched: side 1 has a feature on every node
        assert set(ids.tolist()) <= set(n1.tolist())
        assert not np.array_equal(ids[np.argsort(cnt)], ids)  # node order is not the run-length order


def test_query_counts(OB):
    assert set(E.QUERY_COUNTS) >= {1, 3, 1023, 1024, 1025, 2049}
    F = E.crowd()
    for m in E.QUERY_COUNTS:
        Q = E.local_queries(m)
        assert len(Q["mps"]) == m and Q["md"].shape == (m, 32)
        n, _, _ = OB.search_by_projection_local(F.k2, F.d2, F.bounds, E.SF, Q["ur"], Q["sm"], Q["so"], Q["mps"],
                                                Q["md"], *E.LOCAL_Q_PARAMS[1:])
        assert n >= (1 if m <= 3 else 100), (m, n)


def test_area_bound_windows(OB):
    F = E.tiny(5, 5)
    mps, md, th = E.area_bound_points(F)
    r = 4.0 * th
    lists = [OB.features_in_area(F.k2, F.bounds, p["proj_x"], p["proj_y"], r, -1, 0) for p in mps]
    assert [len(v) for v in lists] == [0, 0, 0, 0, 5, 0]
    minx, maxx, miny, maxy = F.bounds
    # the fifth window covers every cell, the others none
    assert mps["proj_x"][4] - r < minx and mps["proj_x"][4] + r > maxx
    assert mps["proj_y"][4] - r < miny and mps["proj_y"][4] + r > maxy
    assert mps["proj_x"][0] + r < minx and mps["proj_x"][1] - r > maxx
    assert mps["proj_y"][2] + r < miny and mps["proj_y"][3] - r > maxy


def test_bf_cases():
    sizes = {(nq, nt) for nq, nt, kind in E.BF_CASES if kind == "random"}
    assert sizes == {(1, 1), (1, 2), (255, 256), (256, 257), (257, 255), (513, 64)}
    assert any(kind == "equal" for _, _, kind in E.BF_CASES)
    across = 0
    for nq, nt, kind in E.BF_CASES:
        q, t, planted = E.bf_case(nq, nt, kind)
        assert q.shape == (nq, 32) and t.shape == (nt, 32)
        for qi, a, b in planted:
            assert a < b and np.array_equal(t[a], q[qi]) and np.array_equal(t[b], q[qi])
            across += a < 256 <= b
        if kind == "equal":
            assert (q == q[0]).all() and (t == q[0]).all()
    assert across >= 1  # duplicates on both sides of the 256-row tile boundary


def test_extractor_cases(OB):
    w, h = E.min_size(OB)
    p = OB.params()
    OB.levels(p, w, h)
    for bad in ((w - 1, h), (w, h - 1)):
        with pytest.raises(ValueError):
            OB.levels(p, *bad)
    residues = set()
    for name, (_, prm) in E.EXTRACT_CASES.items():
        img = E.extract_image(name)
        lw, lh, _, _ = OB.levels(OB.params(*prm), img.shape[1], img.shape[0])
        residues |= {int(v) % 4 for v in lw[1:]}
    assert residues == {0, 1, 2, 3}
    prms = [prm for _, prm in E.EXTRACT_CASES.values()]
    assert {0, 1, 50000} <= {prm[0] for prm in prms}
    assert any(prm[2] == 1 for prm in prms) and any(prm[1] == 2.0 and prm[2] == 3 for prm in prms)
    assert any(prm[1] == 1.1 and prm[2] == 12 for prm in prms)
    assert E.extract_image("w4096").shape == (240, 4096)
    k, _ = OB.extract(OB.params(*E.EXTRACT_CASES["w4096"][1]), E.extract_image("w4096"))
    assert k["x"][k["octave"] == 0].max() > 4000  # the top of the 12-bit x field of a packed FAST candidate
    blocks = E.extract_image("blocks")
    assert set(np.unique(blocks).tolist()) == {0, 255} and blocks.shape[1] >= 320 and blocks.shape[0] >= 240
    runs = np.diff(np.nonzero(np.diff(blocks[0].astype(int)))[0])
    assert runs.min() >= 3  # blocks of 3..5 px (equal neighbours merge into longer runs)
    # strong corners within EDGE_THRESHOLD of every border: the image has them, the oracle keeps
    # none of them (FAST runs 16 + 3 px inside a level) and keeps keypoints right behind the limit
    img = E.extract_image("border")
    hh, ww = img.shape
    edge = E.EDGE_THRESHOLD
    for strip in (img[:, :edge], img[:, ww - edge:], img[:edge], img[hh - edge:]):
        assert strip.min() == 0 and strip.max() == 255
    k, _ = OB.extract(OB.params(*E.EXTRACT_CASES["border"][1]), img)
    lvl0 = k[k["octave"] == 0]
    dist = (lvl0["x"], ww - 1 - lvl0["x"], lvl0["y"], hh - 1 - lvl0["y"])
    assert all(d.min() >= edge for d in dist) and all((d < 24).sum() >= 3 for d in dist)
    assert dist[0].min() == edge and dist[2].min() == edge  # on the first pixel the extractor may keep


@pytest.mark.parametrize("search,params", E.CASES, ids=[f"{s}-{p}" for s, p in E.CASES])
def test_crowd_matches_and_transliteration(OB, search, params):
    ref = E.run_oracle(OB, "crowd", search, params)
    n = ref[0]
    # four searches reach 100 at their measured case (E.MEASURED), every case of every search 30
    if E.MEASURED.get(search) == params:
        assert n >= 100, n
    assert n >= 30, n
    py = E.run_oracle(OB, "crowd", search, params, translit=True)
    assert py[0] == n
    for a, b in zip(ref[1:], py[1:]):
        np.testing.assert_array_equal(a, b)
    if search == "init":
        m, prev = ref[1], ref[2]
        ok = m >= 0
        F = E.crowd()
        np.testing.assert_array_equal(prev[ok, 0], F.k2["x"][m[ok]])
        np.testing.assert_array_equal(prev[ok, 1], F.k2["y"][m[ok]])
        # the true partner, where one was found
        assert (F.src[ok] == m[ok]).mean() > 0.95


@pytest.mark.parametrize("pair", E.TINY_PAIRS, ids=[f"{a}x{b}" for a, b in E.TINY_PAIRS])
def test_tiny_matches_and_transliteration(OB, pair):
    for search, params in E.CASES:
        ref = E.run_oracle(OB, pair, search, params)
        py = E.run_oracle(OB, pair, search, params, translit=True)
        assert py[0] == ref[0], (search, params)
        for a, b in zip(ref[1:], py[1:]):
            np.testing.assert_array_equal(a, b, err_msg=f"{search} {params}")
        if 0 in pair:
            assert ref[0] == 0
        elif params == E.SEARCHES[search][0]:
            assert ref[0] >= 1, (search, params)  # both frames hold keypoints: the first case of every grid matches
