#!/usr/bin/env python3
"""Time sqlm_bow_transform and sqlm_bow_score (the DBoW2 vocabulary on the GPU) on an MI355X.

A call is host-to-host: staging, upload, the launch, download, the stream
synchronisation and (transform) the host assembly of the BowVectors inside the
entry point, timed with the host clock around it (the method of
scripts/lidar_assoc_bench.py: warm-up, then ``--reps`` windows of ``--calls``
calls; the report is the median window with the smallest and largest as the
spread).

- transform: the synthetic k = 10, L = 6 vocabulary (1,111,111 nodes, ORBvoc's
  shape; orb_scene.make_vocabulary), 2000 features per image — word descriptors
  with 20 bits turned — for 1 and 8 images, levelsup = 4;
- score: a 1,500-word query against 100, 1,000 and 4,000 database vectors of
  1,500 words, which share about a tenth of their words with it.

Every shape's result is compared bit for bit with tests/bow_ref.py. Beside each
is that numpy / Python reference's time on the same box — NOT a DBoW2 time: no
DBoW2 build exists here to compare with, and no time is an acceptance
criterion of this path. The numbers are a record for later work (descriptors
kept on the device between extraction and transform).

Prints one JSON line per shape; needs a GPU (there is no fallback).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sqrtlm-slam_amd"), ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import bow_ref  # noqa: E402
from sqrtlm import orb, orb_scene  # noqa: E402
from sqrtlm._lib import check, lib, ptr  # noqa: E402
from sqrtlm.optimizer import Context  # noqa: E402

N_FEAT, N_WORDS_PER_VECTOR, LEVELSUP = 2000, 1500, 4
TRANSFORM_IMAGES = (1, 8)
SCORE_DB = (100, 1000, 4000)


def windows(fn, args, what, a):
    for _ in range(a.warmup):
        check(fn(*args), what)
    win = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        for _ in range(a.calls):
            fn(*args)
        win.append((time.perf_counter() - t0) / a.calls * 1e3)
    win = np.sort(np.array(win))
    return dict(ms_per_call=round(float(np.median(win)), 4), ms_min=round(float(win[0]), 4),
                ms_max=round(float(win[-1]), 4), calls=a.calls, reps=a.reps)


def features(v, n, seed):
    rng = np.random.default_rng(seed)
    f = v["desc"][rng.choice(np.nonzero(v["is_word"])[0], n)].copy()
    for row in f:
        b = rng.choice(256, 20, replace=False)
        np.bitwise_xor.at(row, b >> 3, (1 << (b & 7)).astype(np.uint8))
    return f


def vector(rng, pool):
    w = np.sort(rng.choice(pool, N_WORDS_PER_VECTOR, replace=False)).astype(np.int32)
    x = rng.random(N_WORDS_PER_VECTOR) + 1e-3
    return w, x / x.sum()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--reps", type=int, default=7, help="timed windows per shape")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    lines = []
    note = "tests/bow_ref.py (numpy / Python) on this host: a correctness reference, not DBoW2; no DBoW2 build exists here"
    with Context(0) as ctx:
        v = orb_scene.make_vocabulary(10, 6, seed=1)
        t0 = time.perf_counter()
        voc = orb.ORBVocabulary(**v, device=0)
        create_ms = (time.perf_counter() - t0) * 1e3
        info = voc.info()
        for n_img in TRANSFORM_IMAGES:
            imgs = [features(v, N_FEAT, 100 + j) for j in range(n_img)]
            t0 = time.perf_counter()
            ref = [bow_ref.transform(v, f, LEVELSUP) for f in imgs]
            ref_ms = (time.perf_counter() - t0) * 1e3
            off = np.arange(n_img + 1, dtype=np.int64) * N_FEAT
            desc = np.concatenate(imgs)
            n = n_img * N_FEAT
            word, node, bw = (np.zeros(n, np.int32) for _ in range(3))
            bv, boff = np.zeros(n), np.zeros(n_img + 1, np.int64)
            args = (ctx._h, voc._h, n_img, ptr(off), ptr(desc), LEVELSUP, ptr(word), ptr(node), ptr(boff), ptr(bw), ptr(bv))
            t = windows(lib().sqlm_bow_transform, args, "sqlm_bow_transform", a)
            same = all(np.array_equal(bw[boff[j]:boff[j + 1]], r[0])
                       and np.array_equal(bow_ref.bits(bv[boff[j]:boff[j + 1]]), bow_ref.bits(r[1]))
                       and np.array_equal(word[off[j]:off[j + 1]], r[2]) and np.array_equal(node[off[j]:off[j + 1]], r[3])
                       for j, r in enumerate(ref))
            lines.append(json.dumps(dict(call="sqlm_bow_transform", k=info["k"], L=info["L"], n_nodes=info["n_nodes"],
                                         n_img=n_img, n_feat=n, levelsup=LEVELSUP, bow_entries=int(boff[-1]),
                                         bit_equal_to_reference=bool(same), **t,
                                         includes="host staging, H2D, 1 launch, D2H, sync, host BowVector assembly",
                                         voc_create_ms_once=round(create_ms, 1), reference_ms=round(ref_ms, 2),
                                         reference_note=note)))
            print(lines[-1], flush=True)
        rng = np.random.default_rng(3)
        pool = 15000  # words drawn from 0..pool: two 1,500-word vectors share about 150
        q = vector(rng, pool)
        db = [vector(rng, pool) for _ in range(max(SCORE_DB))]
        for n_db in SCORE_DB:
            t0 = time.perf_counter()
            ref = [bow_ref.score(q, d) for d in db[:n_db]]
            ref_ms = (time.perf_counter() - t0) * 1e3
            off = np.arange(n_db + 1, dtype=np.int64) * N_WORDS_PER_VECTOR
            dw = np.concatenate([d[0] for d in db[:n_db]])
            dv = np.concatenate([d[1] for d in db[:n_db]])
            s, nc = np.zeros(n_db), np.zeros(n_db, np.int32)
            args = (ctx._h, len(q[0]), ptr(q[0]), ptr(q[1]), n_db, ptr(off), ptr(dw), ptr(dv), ptr(s), ptr(nc))
            t = windows(lib().sqlm_bow_score, args, "sqlm_bow_score", a)
            same = (np.array_equal(bow_ref.bits(s), bow_ref.bits(np.array([r[0] for r in ref])))
                    and nc.tolist() == [r[1] for r in ref])
            lines.append(json.dumps(dict(call="sqlm_bow_score", nq=len(q[0]), n_db=n_db, db_entries=int(off[-1]),
                                         upload_mb=round((dw.nbytes + dv.nbytes) / 1e6, 2),
                                         mean_common=round(float(nc.mean()), 1), bit_equal_to_reference=bool(same), **t,
                                         includes="host staging, H2D of the whole database, 1 launch, D2H, sync",
                                         reference_ms=round(ref_ms, 2), reference_note=note)))
            print(lines[-1], flush=True)
        voc.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
