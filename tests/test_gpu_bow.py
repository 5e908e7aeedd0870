"""sqlm_bow_transform and sqlm_bow_score on the GPU against tests/bow_ref.py.
Both are integer work or one fixed-order double chain, so every comparison is
np.array_equal; doubles are compared through their int64 view (bow_ref.bits),
where -0.0 != 0.0 and the last bit counts."""
import numpy as np
import pytest

import bow_ref as R
from sqrtlm import _lib, orb, orb_scene as S
from sqrtlm.optimizer import Context

pytestmark = pytest.mark.gpu

_cache = {}


def voc_pair(k, L, seed=1, ragged=False, stop=0.0):
    """(arrays, the vocabulary on device 0), built once per shape."""
    key = (k, L, seed, ragged, stop)
    if key not in _cache:
        v = S.make_vocabulary(k, L, seed, ragged=ragged, stop=stop)
        _cache[key] = (v, orb.ORBVocabulary(**v, device=0))
    return _cache[key]


def near_words(v, n, seed, flips=20, random_every=0):
    """n word descriptors with `flips` bits turned (and every random_every-th one random)."""
    rng = np.random.default_rng(seed)
    words = np.nonzero(v["is_word"])[0]
    f = v["desc"][rng.choice(words, n)].copy()
    for row in f:
        b = rng.choice(256, flips, replace=False)
        np.bitwise_xor.at(row, b >> 3, (1 << (b & 7)).astype(np.uint8))
    if random_every:
        f[::random_every] = rng.integers(0, 256, f[::random_every].shape, dtype=np.uint8)
    return f


def assert_image(got, ref, what=""):
    """got = (words, values, node) of ORBVocabulary.transform, ref = bow_ref.transform's tuple."""
    bw, bv, _, node = ref
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[2].dtype == np.int32
    assert np.array_equal(got[0], bw), what
    assert np.array_equal(R.bits(got[1]), R.bits(bv)), what
    assert np.array_equal(got[2], node), what


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("k", [1, 2, 10, 16, 17, 20])
def test_transform_at_the_group_and_wave_edges(gpu_ctx, k, L):
    """16 lanes share a feature (a second pass over the children for k = 17..20),
    4 features a wavefront, 16 a workgroup."""
    v, voc = voc_pair(k, L, seed=10 * k + L, stop=0.05)
    assert voc.info() == dict(k=k, L=L, n_nodes=sum(k ** d for d in range(L + 1)), n_words=k ** L, max_children=k,
                              max_leaf_depth=L, min_leaf_depth=L, device=0)
    for n in (0, 1, 3, 4, 5, 63, 64, 65, 257):
        f = near_words(v, n, n, flips=30, random_every=5)
        for levelsup in (0, 1):
            ref = R.transform(v, f, levelsup)
            assert_image(voc.transform(f, levelsup, ctx=gpu_ctx), ref, (n, levelsup))
            word, node = voc.words(f, levelsup, ctx=gpu_ctx)
            assert np.array_equal(word, ref[2]) and np.array_equal(node, ref[3])


def test_transform_real_shape(gpu_ctx):
    """k = 10, L = 6 — ORBvoc's 1,111,111 nodes — and one frame's 2000 features,
    each a word's descriptor with 20 bits turned. Ties between siblings arise on
    their own at this size."""
    v, voc = voc_pair(10, 6)
    assert voc.info()["n_nodes"] == 1111111 and voc.info()["n_words"] == 10 ** 6
    f = near_words(v, 2000, 2)
    word, node, ties = R.descend_vec(v, f, 4)
    assert ties > 100
    ref = R.transform(v, f, 4)
    assert_image(voc.transform(f, ctx=gpu_ctx), ref)  # levelsup = 4, ORB-SLAM2's value
    got_word, _ = voc.words(f, ctx=gpu_ctx)
    assert np.array_equal(got_word, word) and len(np.unique(node)) > 50
    _cache.pop((10, 6, 1, False, 0.0))[1].close()  # 50 MB of device memory nobody else needs


def test_transform_ragged_tree(gpu_ctx):
    """Single children, fewer than k children and words above depth L: groups of
    one wavefront finish at different depths."""
    L = 4
    v, voc = voc_pair(6, L, seed=5, ragged=True, stop=0.05)
    info = voc.info()
    assert info["min_leaf_depth"] == 1 and info["max_leaf_depth"] == L and info["max_children"] == 6
    f = near_words(v, 300, 4, flips=10, random_every=3)
    first, _, _ = R.tree(v)
    assert (np.diff(first) == 1).any()
    depth = np.zeros(len(v["parent"]), int)
    for i in range(1, len(depth)):
        depth[i] = depth[v["parent"][i]] + 1
    seen_root = seen_early = False
    for levelsup in (0, 1, 2, 4, L, L + 2):
        ref = R.transform(v, f, levelsup)
        assert_image(voc.transform(f, levelsup, ctx=gpu_ctx), ref, levelsup)
        word, node = voc.words(f, levelsup, ctx=gpu_ctx)
        assert np.array_equal(word, ref[2])
        kept = ref[3][ref[3] >= 0]
        seen_root |= bool((kept == 0).all()) and levelsup >= L
        seen_early |= bool((depth[kept] < L - levelsup).any())  # node = a leaf above depth L - levelsup
    assert seen_root and seen_early


def test_crafted_tie_goes_to_the_first_child(gpu_ctx):
    v = S.make_vocabulary(3, 2, seed=9)
    # pre-order ids: the root's children are 1, 5, 9 and node 1's are 2, 3, 4
    assert v["parent"].tolist()[:6] == [0, 0, 1, 1, 1, 0]
    v["desc"][5] = v["desc"][1]
    v["desc"][9] = v["desc"][1]
    v["desc"][3] = v["desc"][2]
    f = np.stack([v["desc"][1] ^ v["desc"][2], v["desc"][2], v["desc"][1]])
    with orb.ORBVocabulary(**v, device=0) as voc:
        word, node = voc.words(f, 1, ctx=gpu_ctx)
        ref = R.descend_loop(v, f, 1)
    assert np.array_equal(word, ref[0]) and np.array_equal(node, ref[1]) and ref[2] >= 3
    assert node[1] == 1 and word[1] == 0  # three equal children at the root, two at node 1: the first each time


def test_stop_words(gpu_ctx):
    v, voc = voc_pair(5, 3, seed=6, stop=0.4)
    f = near_words(v, 200, 6)
    ref = R.transform(v, f, 1)
    got = voc.transform(f, 1, ctx=gpu_ctx)
    assert_image(got, ref)
    word, node = voc.words(f, 1, ctx=gpu_ctx)
    stopped = ref[2] < 0
    assert stopped.any() and not stopped.all()
    assert (word[stopped] == -1).all() and (node[stopped] == -1).all() and (node[~stopped] >= 0).all()
    assert (R.word_weights(v)[got[0]] > 0).all()  # no stop word in the vector
    # an image of stopped features only, alone and between two others: an empty vector, nothing divided
    only = f[stopped]
    for batch, at in (([only], 0), ([f[:50], only, f[50:90]], 1)):
        out = voc.transform_many(batch, 1, ctx=gpu_ctx)
        assert len(out[at][0]) == 0 and len(out[at][1]) == 0 and (out[at][2] == -1).all()
        assert len(out[at][2]) == len(only)
        for img, o in zip(batch, out):
            assert_image(o, R.transform(v, img, 1))


def test_repeated_word_adds_its_weight_each_time(gpu_ctx):
    """Seven features on a word of weight 0.1 and one on a word of weight 0.3:
    the vector carries 0.1 added seven times, not 7 * 0.1."""
    v = S.make_vocabulary(2, 1, seed=5)
    v["weight"][1:] = [0.1, 0.3]
    f = np.concatenate([np.repeat(v["desc"][1:2], 7, 0), v["desc"][2:3]])
    with orb.ORBVocabulary(**v, device=0) as voc:
        words, values, node = voc.transform(f, 0, ctx=gpu_ctx)
    ref = R.transform(v, f, 0)
    assert ref[2].tolist() == [0] * 7 + [1] and node.tolist() == [1] * 7 + [2]
    assert words.tolist() == [0, 1] and np.array_equal(R.bits(values), R.bits(ref[1]))
    _, product = R.bow_vector(ref[2], R.word_weights(v), repeat_as_product=True)
    assert not np.array_equal(R.bits(values), R.bits(product))


def test_batch_invariance(gpu_ctx):
    """An image's result does not depend on the batch around it."""
    v, voc = voc_pair(10, 3, seed=8, ragged=True, stop=0.05)
    imgs = [near_words(v, n, 20 + n, flips=25, random_every=4) for n in (37, 0, 64, 1, 130)]
    alone = [voc.transform(f, 1, ctx=gpu_ctx) for f in imgs]
    for f, a in zip(imgs, alone):
        assert_image(a, R.transform(v, f, 1))
    batch = voc.transform_many(imgs, 1, ctx=gpu_ctx)
    back = voc.transform_many(imgs[::-1], 1, ctx=gpu_ctx)[::-1]
    for a, b, c in zip(alone, batch, back):
        for x, y, z in zip(a, b, c):  # words, values, node: the same bytes
            assert x.dtype == y.dtype == z.dtype and x.tobytes() == y.tobytes() == z.tobytes()


def test_node_feeds_search_by_bow(gpu_ctx):
    """node[] is the FeatureVector in the form BowFrame takes: SearchByBoW over
    it gives the matches it gives over the reference's node ids."""
    v, voc = voc_pair(5, 3, seed=6, stop=0.4)
    rng = np.random.default_rng(12)
    n = 300
    d1 = near_words(v, n, 30, flips=6)
    d2 = d1.copy()
    for row in d2:
        b = rng.choice(256, 4, replace=False)
        np.bitwise_xor.at(row, b >> 3, (1 << (b & 7)).astype(np.uint8))
    d2 = np.ascontiguousarray(d2[rng.permutation(n)])

    def keys(seed):
        r = np.random.default_rng(seed)
        k = np.zeros(n, orb.KP_DTYPE)
        k["x"], k["y"] = r.uniform(0, 1241, n), r.uniform(0, 376, n)
        k["size"], k["angle"], k["octave"] = 31.0, r.uniform(0, 360, n), r.integers(0, 8, n)
        return k

    k1, k2 = keys(1), keys(2)
    mp1, bad1 = S.bow_points(n, 1)
    mp2, bad2 = S.bow_points(n, 2, base=10000)
    (_, _, g1), (_, _, g2) = voc.transform_many([d1, d2], 1, ctx=gpu_ctx)
    r1, r2 = R.descend_vec(v, d1, 1)[1], R.descend_vec(v, d2, 1)[1]
    assert (r1 < 0).any() and len(np.unique(r1)) > 10
    m = orb.ORBmatcher(0.75, False, ctx=gpu_ctx)
    n_g, out_g = m.SearchByBoW(orb.BowFrame(k1, d1, g1, mp1, bad1), orb.BowFrame(k2, d2, g2, mp2, bad2))
    n_r, out_r = m.SearchByBoW(orb.BowFrame(k1, d1, r1, mp1, bad1), orb.BowFrame(k2, d2, r2, mp2, bad2))
    assert n_g == n_r and n_r > 50 and np.array_equal(out_g, out_r)
    assert g1.dtype == np.int32 and orb.BowFrame(k1, d1, g1).node is not None


# ---- score ----
def random_vector(rng, n, n_words=20000):
    w = np.sort(rng.choice(n_words, n, replace=False)).astype(np.int32)
    x = rng.random(n) + 1e-3
    return w, x / x.sum()


@pytest.fixture(scope="module")
def score_set():
    """A 1500-word query and 1000 database vectors: lengths 0, 1 and 1500 among
    them, one equal to the query, one sharing no word with it. The reference
    scores are computed once."""
    rng = np.random.default_rng(7)
    q = random_vector(rng, 1500)
    lengths = rng.integers(0, 80, 1000)
    lengths[[0, 5, 17, 62, 63, 64, 65, 999]] = [1500, 0, 1, 1500, 0, 1500, 1, 1500]
    db = [random_vector(rng, n) for n in lengths]
    db[3] = (q[0].copy(), q[1].copy())
    free = np.setdiff1d(np.arange(20000), q[0])[:40].astype(np.int32)
    db[4] = (free, np.full(40, 1 / 40))
    db[6] = (q[0][::3].copy(), rng.random(500))  # a subset: every word common
    ref = [R.score(q, d) for d in db]
    return q, db, np.array([r[0] for r in ref]), np.array([r[1] for r in ref], np.int32)


@pytest.fixture(scope="module")
def small_voc():
    return voc_pair(2, 2)[1]  # score needs no tree: any vocabulary carries the call


@pytest.mark.parametrize("n_db", [0, 1, 63, 64, 65, 1000])
def test_score_shapes(gpu_ctx, small_voc, score_set, n_db):
    q, db, ref_s, ref_n = score_set
    s, n = small_voc.score_many(q, db[:n_db], ctx=gpu_ctx)
    assert s.shape == (n_db,) and n.shape == (n_db,) and n.dtype == np.int32
    assert np.array_equal(R.bits(s), R.bits(ref_s[:n_db])) and np.array_equal(n, ref_n[:n_db])


def test_score_values(gpu_ctx, small_voc, score_set):
    q, db, ref_s, ref_n = score_set
    s, n = small_voc.score_many(q, db, ctx=gpu_ctx)
    assert np.array_equal(R.bits(s), R.bits(ref_s)) and np.array_equal(n, ref_n)
    # the query against itself: the reference's bits, whatever they are, and every word common
    assert R.bits(s[3:4])[0] == R.bits(ref_s[3:4])[0] and n[3] == 1500 and abs(s[3] - 1.0) < 1e-12
    # no common word, an empty vector: -0.0, sign bit included
    minus_zero = R.bits(np.array([-0.0]))[0]
    assert n[4] == 0 and n[5] == 0 and R.bits(s[4:6]).tolist() == [minus_zero, minus_zero]
    assert n[6] == 500 and (ref_n > 0).sum() > 100
    # one pair through score(): vi is the first argument's value
    assert small_voc.score(q, db[0], ctx=gpu_ctx) == ref_s[0]
    assert R.bits(np.array([small_voc.score(db[0], q, ctx=gpu_ctx)]))[0] == R.bits(np.array([R.score(db[0], q)[0]]))[0]


def test_score_empty_query(gpu_ctx, small_voc, score_set):
    _, db, _, _ = score_set
    empty = (np.zeros(0, np.int32), np.zeros(0))
    s, n = small_voc.score_many(empty, db[:70], ctx=gpu_ctx)
    assert (R.bits(s) == R.bits(np.array([-0.0]))[0]).all() and not n.any()
    s, n = small_voc.score_many(empty, [], ctx=gpu_ctx)
    assert len(s) == 0 and len(n) == 0
    s, n = small_voc.score_many(score_set[0], [empty, empty], ctx=gpu_ctx)
    assert (R.bits(s) == R.bits(np.array([-0.0]))[0]).all() and not n.any()


@pytest.mark.parametrize("nq", [4096, 4097])
def test_score_query_at_the_lds_limit(gpu_ctx, small_voc, nq):
    """Up to 4096 query entries are kept in LDS; a longer query is read from memory."""
    rng = np.random.default_rng(nq)
    q = random_vector(rng, nq)
    db = [random_vector(rng, n) for n in (0, 1, 33, 900)] + [(q[0].copy(), q[1].copy()), (q[0][-5:].copy(), q[1][:5].copy())]
    ref = [R.score(q, d) for d in db]
    s, n = small_voc.score_many(q, db, ctx=gpu_ctx)
    assert np.array_equal(R.bits(s), R.bits(np.array([r[0] for r in ref]))) and n.tolist() == [r[1] for r in ref]
    assert n[4] == nq and n[5] == 5


def test_score_without_n_common_and_argument_checks(gpu_ctx, small_voc, score_set):
    q, db, ref_s, _ = score_set
    L, p = _lib.lib(), _lib.ptr
    off = np.array([0, len(db[2][0])], np.int64)
    s = np.zeros(1)
    assert L.sqlm_bow_score(gpu_ctx._h, len(q[0]), p(q[0]), p(q[1]), 1, p(off), p(db[2][0]), p(db[2][1]), p(s), None) == 0
    assert R.bits(s)[0] == R.bits(ref_s[2:3])[0]
    # word arrays must be strictly ascending and >= 0; offsets from 0, ascending
    w = np.array([3, 9, 9], np.int32)
    x = np.full(3, 1 / 3)
    off3 = np.array([0, 3], np.int64)
    for qw, dw, o in ((w, q[0][:3], off3), (q[0][:3], w, off3), (q[0][:3], w[::-1].copy(), off3),
                      (np.array([-1, 2, 3], np.int32), q[0][:3], off3), (q[0][:3], q[0][:3], np.array([1, 3], np.int64)),
                      (q[0][:3], q[0][:3], np.array([0, -3], np.int64))):
        assert L.sqlm_bow_score(gpu_ctx._h, 3, p(qw), p(x), 1, p(o), p(dw), p(x), p(s), None) == -1
    # a descending pair of words that straddles two database vectors is fine
    two = np.array([0, 2, 3], np.int64)
    dw = np.array([5, 9, 7], np.int32)
    s2 = np.zeros(2)
    assert L.sqlm_bow_score(gpu_ctx._h, 3, p(q[0][:3]), p(x), 2, p(two), p(dw), p(x), p(s2), None) == 0
    # transform: no vocabulary, bad offsets
    v, voc = voc_pair(2, 2)
    f = near_words(v, 4, 1)
    i32, f64, boff = np.zeros(4, np.int32), np.zeros(4), np.zeros(2, np.int64)
    ok = np.array([0, 4], np.int64)
    args = (p(f), 1, p(i32), p(i32.copy()), p(boff), p(i32.copy()), p(f64))
    assert L.sqlm_bow_transform(gpu_ctx._h, None, 1, p(ok), *args) == -1
    assert L.sqlm_bow_transform(gpu_ctx._h, voc._h, 1, p(np.array([1, 4], np.int64)), *args) == -1
    assert L.sqlm_bow_transform(gpu_ctx._h, voc._h, 1, p(np.array([0, -4], np.int64)), *args) == -1
    assert L.sqlm_bow_transform(gpu_ctx._h, voc._h, -1, p(ok), *args) == -1
    assert L.sqlm_bow_transform(gpu_ctx._h, voc._h, 1, p(ok), None, 1, *args[2:]) == -1
    assert L.sqlm_bow_transform(gpu_ctx._h, voc._h, 1, p(ok), *args) == 0
    assert L.sqlm_bow_transform(gpu_ctx._h, voc._h, 0, p(ok), None, 1, None, None, p(boff), None, None) == 0  # n_img = 0


def test_one_vocabulary_two_contexts_and_small_after_large(gpu_ctx):
    """The vocabulary belongs to the device: two contexts use one copy. The
    staging buffers belong to the context: a small call after a large one reads
    its own results."""
    v, voc = voc_pair(10, 3, seed=8, ragged=True, stop=0.05)
    big, small = near_words(v, 1500, 40, random_every=6), near_words(v, 3, 41)
    ref_big, ref_small = R.transform(v, big, 2), R.transform(v, small, 2)
    with Context(0) as other:
        a = voc.transform(big, 2, ctx=gpu_ctx)
        b = voc.transform(big, 2, ctx=other)
        assert_image(a, ref_big)
        assert_image(b, ref_big)
        assert_image(voc.transform(small, 2, ctx=other), ref_small)
        assert_image(voc.transform(small, 2, ctx=gpu_ctx), ref_small)
        # the vectors the transform made score the same on both contexts, and after a larger score call
        va, vs = (a[0], a[1]), (ref_small[0], ref_small[1])
        many = voc.score_many(va, [va] * 40 + [vs], ctx=other)
        ref = R.score(va, vs)
        for c in (other, gpu_ctx):
            s, n = voc.score_many(va, [vs], ctx=c)
            assert R.bits(s)[0] == R.bits(np.array([ref[0]]))[0] == R.bits(many[0][-1:])[0] and n[0] == ref[1]
    # its own context, made on demand on the vocabulary's device
    assert_image(voc.transform(small, 2), ref_small)
