"""tests/bow_ref.py against itself, and the vocabulary generator and text
format it is used with: the literal descent and the per-level one agree, a
saved vocabulary loads back bit for bit, and the repeated-add rule of the
BowVector is not n * w."""
import numpy as np
import pytest

import bow_ref as R
from sqrtlm import orb, orb_scene as S


def _feats(voc, n, seed, flips=20):
    """Word descriptors with `flips` bits turned, and a few random ones."""
    rng = np.random.default_rng(seed)
    words = np.nonzero(voc["is_word"])[0]
    f = voc["desc"][rng.choice(words, n)].copy()
    for row in f:
        b = rng.choice(256, flips, replace=False)
        np.bitwise_xor.at(row, b >> 3, (1 << (b & 7)).astype(np.uint8))
    f[::7] = rng.integers(0, 256, f[::7].shape, dtype=np.uint8)
    return f


@pytest.mark.parametrize("k,L,ragged", [(1, 3, False), (2, 4, True), (3, 3, True), (10, 2, False), (17, 2, True),
                                        (20, 1, False)])
def test_generator_obeys_the_layout(k, L, ragged):
    v = S.make_vocabulary(k, L, seed=k + L, ragged=ragged, stop=0.1)
    p, n = v["parent"], len(v["parent"])
    assert p[0] == 0 and (p[1:] < np.arange(1, n)).all() and (p[1:] >= 0).all()
    first, kids, word_id = R.tree(v)
    cnt = np.diff(first)
    assert cnt.max() <= k and ((cnt == 0) == (v["is_word"] > 0)).all()
    assert (v["weight"][v["is_word"] == 0] == 0).all()
    if not ragged:
        assert n == sum(k ** d for d in range(L + 1)) and (cnt[cnt > 0] == k).all()
    again = S.make_vocabulary(k, L, seed=k + L, ragged=ragged, stop=0.1)
    assert all(np.array_equal(v[a], again[a]) for a in ("parent", "is_word", "desc", "weight"))  # seeded


def test_ragged_generator_has_single_children_and_early_leaves():
    v = S.make_vocabulary(4, 4, seed=3, ragged=True)
    first, _, _ = R.tree(v)
    cnt = np.diff(first)
    depth = np.zeros(len(cnt), int)
    for i in range(1, len(cnt)):
        depth[i] = depth[v["parent"][i]] + 1
    assert (cnt == 1).any() and ((cnt > 1) & (cnt < 4)).any()
    assert ((v["is_word"] > 0) & (depth < 4)).any() and ((v["is_word"] > 0) & (depth == 4)).any()


@pytest.mark.parametrize("k,L,seed", [(2, 4, 1), (3, 3, 2), (5, 3, 3), (20, 2, 4), (1, 3, 5)])
def test_loop_and_vectorised_descent_agree(k, L, seed):
    v = S.make_vocabulary(k, L, seed, ragged=True, stop=0.15)
    f = _feats(v, 60, seed, flips=12)
    for levelsup in (0, 1, 4, L, L + 2):
        a = R.descend_loop(v, f, levelsup)
        b = R.descend_vec(v, f, levelsup)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        ta, tb = R.transform(v, f, levelsup, vectorised=False), R.transform(v, f, levelsup, vectorised=True)
        assert all(np.array_equal(x, y) for x, y in zip(ta[:1] + ta[2:], tb[:1] + tb[2:]))
        assert np.array_equal(R.bits(ta[1]), R.bits(tb[1]))


def test_stop_words_leave_both_vectors():
    v = S.make_vocabulary(5, 3, seed=6, stop=0.4)
    f = _feats(v, 80, 6)
    bw, bv, word, node = R.transform(v, f, 1)
    assert (word < 0).any() and (word >= 0).any() and np.array_equal(word < 0, node < 0)
    assert (R.word_weights(v)[bw] > 0).all() and set(bw.tolist()) == set(word[word >= 0].tolist())
    free = R.transform(dict(v, weight=np.where(v["is_word"] > 0, 1.0, 0.0)), f, 1)
    assert (free[2] >= 0).all() and np.array_equal(free[2][word >= 0], word[word >= 0])


def test_first_child_wins_a_tie():
    v = S.make_vocabulary(3, 1, seed=9)
    v["desc"][2] = v["desc"][1]  # children 1 and 2 are equally far from everything
    f = v["desc"][1:2].copy()
    for fn in (R.descend_loop, R.descend_vec):
        word, node, ties = fn(v, f, 0)
        assert word[0] == 0 and node[0] == 1 and ties == 1


def test_text_round_trip(tmp_path):
    v = S.make_vocabulary(3, 3, seed=11, ragged=True, stop=0.2)
    v["weight"][np.nonzero(v["is_word"])[0][0]] = 0.1 + 0.2  # a value whose shortest decimal form needs 17 digits
    voc = orb.ORBVocabulary(**v, upload=False)
    path = tmp_path / "voc.txt"
    voc.save_text(path)
    back = orb.load_vocabulary_text(path)
    assert (back["k"], back["L"], back["scoring"], back["weighting"]) == (3, 3, 0, 0)
    for a in ("parent", "is_word", "desc"):
        assert back[a].dtype == getattr(voc, a).dtype and np.array_equal(back[a], v[a]), a
    assert np.array_equal(R.bits(back["weight"]), R.bits(v["weight"]))
    # blank lines, a trailing one included, are skipped
    text = path.read_text().splitlines()
    path.write_text("\n".join(text[:3] + [""] + text[3:]) + "\n\n")
    again = orb.ORBVocabulary.load_text(path, upload=False)
    assert np.array_equal(again.parent, v["parent"]) and np.array_equal(R.bits(again.weight), R.bits(v["weight"]))
    assert len(again.parent) == len(text)  # header + one line per node after the root


def test_repeated_word_is_added_not_multiplied():
    """A word seen n times has its weight added n times: 0.1 six times is not 6 * 0.1."""
    weights = np.array([0.1, 0.7])
    acc = 0.0
    for _ in range(6):
        acc += 0.1
    assert acc != 6 * 0.1
    words = np.array([0] * 6 + [1], np.int32)
    w, x = R.bow_vector(words, weights)
    wp, xp = R.bow_vector(words, weights, repeat_as_product=True)
    assert w.tolist() == wp.tolist() == [0, 1]
    assert x[0] == acc / (acc + 0.7) and xp[0] == (6 * 0.1) / (6 * 0.1 + 0.7)
    assert not np.array_equal(R.bits(x), R.bits(xp))


def test_score_of_the_reference():
    a = (np.array([1, 4, 9], np.int32), np.array([0.5, 0.25, 0.25]))
    b = (np.array([0, 4, 9, 11], np.int32), np.array([0.25, 0.25, 0.125, 0.375]))
    s, n = R.score(a, b)
    assert n == 2 and s == -((abs(0.25 - 0.25) - 0.25 - 0.25) + (abs(0.25 - 0.125) - 0.25 - 0.125)) / 2.0
    s, n = R.score(a, (np.array([2, 3], np.int32), np.array([0.5, 0.5])))
    assert n == 0 and s == 0.0 and np.signbit(s)  # no common word: -0.0
    assert R.score(a, a) == (1.0, 3)
