"""The DBoW2 vocabulary in plain numpy / Python: what sqlm_bow_transform and
sqlm_bow_score must equal bit for bit.

A vocabulary is the dict of sqlm_voc_create's arrays (k, L, parent, is_word,
desc, weight): node 0 is the root, a node's children are the nodes that name it
as parent in ascending id, word ids number the is_word nodes in ascending id.

- the descent of one feature: from the root, at every node to the child with
  the smallest Hamming distance, the first such child on ties, until a node
  without children; ``descend_loop`` is that sentence literally, one feature
  and one child at a time, ``descend_vec`` does a level of all features at
  once. The FeatureVector node is the node chosen at depth L - levelsup: the
  root when that is <= 0, the leaf itself when the leaf sits above that depth.
- the BowVector of an image: every feature whose word weighs more than 0 adds
  the weight to its word's entry, in feature order, one addition per
  occurrence; the entries, in ascending word id, are then divided by the sum
  of their magnitudes, itself summed in that order (if it is > 0).
- the L1 score of two vectors: over the common words in ascending id,
  sum += |v - w| - |v| - |w|; the score is -sum / 2.

Python floats are IEEE doubles and every sum here is a plain left-to-right
loop, so the order of operations is the definition's."""
import numpy as np

POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)


def tree(voc):
    """(first, kids, word_id): node i's children are kids[first[i]:first[i+1]]."""
    parent = np.asarray(voc["parent"], np.int64)
    n = len(parent)
    cnt = np.bincount(parent[1:], minlength=n)
    first = np.concatenate([[0], np.cumsum(cnt)])
    kids = np.argsort(parent[1:], kind="stable") + 1
    is_word = np.asarray(voc["is_word"]) > 0
    word_id = np.where(is_word, np.cumsum(is_word) - 1, -1)
    return first, kids, word_id


def hamming(a, b):
    return int(POPCOUNT[np.bitwise_xor(a, b)].sum())


def descend_loop(voc, feats, levelsup):
    """(word, node, ties) per feature, -1 / -1 for stop words; ties = the number
    of descent steps whose smallest distance two children share."""
    first, kids, word_id = tree(voc)
    desc, weight, L = np.asarray(voc["desc"], np.uint8), voc["weight"], voc["L"]
    feats = np.asarray(feats, np.uint8).reshape(-1, 32)
    word = np.full(len(feats), -1, np.int32)
    node = np.full(len(feats), -1, np.int32)
    ties = 0
    for i, f in enumerate(feats):
        cur, level = 0, 0
        sel = 0 if L - levelsup <= 0 else None
        while first[cur + 1] > first[cur]:
            level += 1
            best, best_d, n_best = None, None, 0
            for c in kids[first[cur]:first[cur + 1]]:
                d = hamming(f, desc[c])
                if best is None or d < best_d:
                    best, best_d, n_best = c, d, 1
                elif d == best_d:
                    n_best += 1
            ties += n_best > 1
            cur = best
            if level == L - levelsup:
                sel = cur
        if sel is None:
            sel = cur
        if weight[cur] > 0:
            word[i], node[i] = word_id[cur], sel
    return word, node, ties


def descend_vec(voc, feats, levelsup):
    """The same, one tree level of every feature at a time."""
    first, kids, word_id = tree(voc)
    desc, weight, L = np.asarray(voc["desc"], np.uint8), np.asarray(voc["weight"]), voc["L"]
    feats = np.asarray(feats, np.uint8).reshape(-1, 32)
    n = len(feats)
    cur = np.zeros(n, np.int64)
    sel = np.full(n, 0 if L - levelsup <= 0 else -1, np.int64)
    ties = 0
    level = 0
    while True:
        cnt = first[cur + 1] - first[cur]
        go = np.nonzero(cnt > 0)[0]
        if len(go) == 0:
            break
        level += 1
        best = np.zeros(len(go), np.int64)
        best_d = np.full(len(go), 1 << 30, np.int64)
        n_best = np.zeros(len(go), np.int64)
        for j in range(int(cnt[go].max())):
            has = cnt[go] > j
            c = kids[np.where(has, first[cur[go]] + j, 0)]
            d = POPCOUNT[desc[c] ^ feats[go]].sum(1)
            better = has & (d < best_d)
            n_best = np.where(better, 1, n_best + (has & (d == best_d)))
            best = np.where(better, c, best)
            best_d = np.where(better, d, best_d)
        ties += int((n_best > 1).sum())
        cur[go] = best
        if level == L - levelsup:
            sel[go] = best
    sel = np.where(sel < 0, cur, sel)
    keep = weight[cur] > 0
    return (np.where(keep, word_id[cur], -1).astype(np.int32), np.where(keep, sel, -1).astype(np.int32), ties)


def word_weights(voc):
    return np.asarray(voc["weight"], np.float64)[np.asarray(voc["is_word"]) > 0]


def bow_vector(words, weights, repeat_as_product=False):
    """The BowVector of one image from its features' words (-1: none) and the
    weight of every word id: (words ascending int32, values float64).
    repeat_as_product builds the other thing — n * w for a word seen n times —
    for the tests that show the two differ."""
    acc, seen = {}, {}
    for w in words:
        w = int(w)
        if w < 0:
            continue
        x = float(weights[w])
        acc[w] = acc[w] + x if w in acc else x
        seen[w] = seen.get(w, 0) + 1
    ids = sorted(acc)
    vals = [seen[w] * float(weights[w]) for w in ids] if repeat_as_product else [acc[w] for w in ids]
    norm = 0.0
    for v in vals:
        norm += abs(v)
    if norm > 0.0:
        vals = [v / norm for v in vals]
    return np.array(ids, np.int32), np.array(vals, np.float64)


def transform(voc, feats, levelsup=4, vectorised=True):
    """(words, values, word_per_feature, node_per_feature)."""
    word, node, _ = (descend_vec if vectorised else descend_loop)(voc, feats, levelsup)
    bw, bv = bow_vector(word, word_weights(voc))
    return bw, bv, word, node


def score(v1, v2):
    """(L1 score, number of common words) of two BowVectors (words, values)."""
    w1, x1 = np.asarray(v1[0]).tolist(), np.asarray(v1[1], np.float64).tolist()
    w2, x2 = np.asarray(v2[0]).tolist(), np.asarray(v2[1], np.float64).tolist()
    i = j = common = 0
    s = 0.0
    while i < len(w1) and j < len(w2):
        if w1[i] == w2[j]:
            vi, wi = x1[i], x2[j]
            s += abs(vi - wi) - abs(vi) - abs(wi)
            common += 1
            i += 1
            j += 1
        elif w1[i] < w2[j]:
            i += 1
        else:
            j += 1
    return -s / 2.0, common


def bits(a):
    """Doubles as int64, so that -0.0 != 0.0 and the last bit counts."""
    return np.ascontiguousarray(a, np.float64).view(np.int64)
