"""Pure Python / NumPy restatement of the reference's BoW scoring and keyframe
database, for the tests of orbv_score and orbdb_*:

  - the six DBoW2 scorings (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-311),
  - KeyFrameDatabase with per-word Python lists as its inverted file
    (src/KeyFrameDatabase.cc:76-109) and the two Detect functions (:112-345).

Doubles are Python floats (IEEE double, one operation at a time, in the
reference's order; log and sqrt are the host libm's through `math`), and
np.float32 stands wherever the reference has `float`. BowVectors are
(words, values) pairs of ascending uint32 words and float64 values.
"""
from __future__ import annotations

import math
import sys

import numpy as np

L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)
LOG_EPS = math.log(sys.float_info.epsilon)  # GeneralScoring::LOG_EPS = log(DBL_EPSILON)


def _log(x: float) -> float:
    if x == 0:
        return -math.inf
    return math.log(x) if x > 0 else math.nan


def _shared(w1, v1, w2, v2):
    """(vi, wi) of the words both vectors hold, in ascending word order: the pairs the
    reference's walk (with its lower_bound jumps) visits in its equal-word branch."""
    i = j = 0
    n1, n2 = len(w1), len(w2)
    while i < n1 and j < n2:
        if w1[i] == w2[j]:
            yield float(v1[i]), float(v2[j])
            i += 1
            j += 1
        elif w1[i] < w2[j]:
            i += 1
        else:
            j += 1


def score(scoring: int, a, b) -> float:
    (w1, v1), (w2, v2) = a, b
    s = 0.0
    if scoring == L1_NORM:
        for vi, wi in _shared(w1, v1, w2, v2):
            s += math.fabs(vi - wi) - math.fabs(vi) - math.fabs(wi)
        return -s / 2.0
    if scoring == L2_NORM:
        for vi, wi in _shared(w1, v1, w2, v2):
            s += vi * wi
        return 1.0 if s >= 1 else 1.0 - math.sqrt(1.0 - s)
    if scoring == CHI_SQUARE:
        for vi, wi in _shared(w1, v1, w2, v2):
            if vi + wi != 0.0:
                s += vi * wi / (vi + wi)
        return 2. * s
    if scoring == KL:
        i = j = 0
        n1, n2 = len(w1), len(w2)
        while i < n1 and j < n2:
            vi, wi = float(v1[i]), float(v2[j])
            if w1[i] == w2[j]:
                if vi != 0 and wi != 0:
                    s += vi * _log(vi / wi)
                i += 1
                j += 1
            elif w1[i] < w2[j]:
                s += vi * (_log(vi) - LOG_EPS)
                i += 1
            else:
                j += 1
        while i < n1:
            vi = float(v1[i])
            if vi != 0:
                s += vi * (_log(vi) - LOG_EPS)
            i += 1
        return s
    if scoring == BHATTACHARYYA:
        for vi, wi in _shared(w1, v1, w2, v2):
            s += math.sqrt(vi * wi)
        return s
    if scoring == DOT_PRODUCT:
        for vi, wi in _shared(w1, v1, w2, v2):
            s += vi * wi
        return s
    raise ValueError(scoring)


class RefKF:
    """What the database reads and writes on a KeyFrame / Frame."""
    _next = 0

    def __init__(self, bow, mnId=None):
        self.bow = (np.asarray(bow[0], np.uint32), np.asarray(bow[1], np.float64))
        if mnId is None:
            mnId = RefKF._next
            RefKF._next += 1
        self.mnId = mnId
        self.mnLoopQuery = self.mnRelocQuery = -1
        self.mnLoopWords = self.mnRelocWords = 0
        self.mLoopScore = np.float32(0)
        self.mRelocScore = np.float32(0)  # the library's definition of the uninitialised float
        self.connected = set()   # GetConnectedKeyFrames()
        self.covisibles = []     # GetBestCovisibilityKeyFrames(10)


class RefDatabase:
    def __init__(self):
        self.inv = {}  # word -> list of keyframes, insertion order (mvInvertedFile)
        self.query_id = 1 << 40  # each Detect call is a fresh query id

    def add(self, kf):
        for w in kf.bow[0]:
            self.inv.setdefault(int(w), []).append(kf)

    def erase(self, kf):
        for w in kf.bow[0]:
            lst = self.inv.get(int(w), [])
            for k, x in enumerate(lst):
                if x is kf:
                    del lst[k]
                    break

    def clear(self):
        self.inv = {}

    # ---- the first half of both Detect functions
    def _sharing(self, q_bow, loop, connected):
        qid = self.query_id
        self.query_id += 1
        lst = []
        for w in q_bow[0]:
            for kf in self.inv.get(int(w), []):
                if loop:
                    if kf.mnLoopQuery != qid:
                        kf.mnLoopWords = 0
                        if kf not in connected:
                            kf.mnLoopQuery = qid
                            lst.append(kf)
                    kf.mnLoopWords += 1
                else:
                    if kf.mnRelocQuery != qid:
                        kf.mnRelocWords = 0
                        kf.mnRelocQuery = qid
                        lst.append(kf)
                    kf.mnRelocWords += 1
        return qid, lst

    def query(self, q_bow, loop, connected=(), min_score=0.0):
        """lScoreAndMatch as [(si, kf)], minCommonWords, maxCommonWords, the query id."""
        min_score = np.float32(min_score)
        qid, lst = self._sharing(q_bow, loop, set(connected))
        if not lst:
            return [], 0, 0, qid
        words = (lambda k: k.mnLoopWords) if loop else (lambda k: k.mnRelocWords)
        max_common = 0
        for kf in lst:
            if words(kf) > max_common:
                max_common = words(kf)
        min_common = int(np.float32(max_common) * np.float32(0.8))
        out = []
        for kf in lst:
            if words(kf) > min_common:
                si = np.float32(score(L1_NORM, q_bow, kf.bow))
                if loop:
                    kf.mLoopScore = si
                    if si >= min_score:
                        out.append((si, kf))
                else:
                    kf.mRelocScore = si
                    out.append((si, kf))
        return out, min_common, max_common, qid

    def hits(self, q_bow, kfs_by_slot, excluded=()):
        """Per slot (common, first_word, score or -1.0) and max_common, as orbdb_query_batch
        defines them; kfs_by_slot: the live keyframe of each slot or None."""
        ex = set(excluded)
        qw = set(int(w) for w in q_bow[0])
        rows = []
        for kf in kfs_by_slot:
            sh = [] if kf is None or kf in ex else [int(w) for w in kf.bow[0] if int(w) in qw]
            rows.append((len(sh), min(sh) if sh else 0))
        max_common = max([c for c, _ in rows], default=0)
        min_common = int(np.float32(max_common) * np.float32(0.8))
        out = np.zeros(len(rows), np.dtype([("common", "<i4"), ("first_word", "<u4"), ("score", "<f8")]))
        for s, (c, fw) in enumerate(rows):
            out[s] = (c, fw, score(L1_NORM, q_bow, kfs_by_slot[s].bow) if c > min_common else -1.0)
        return out, max_common

    # ---- the second half
    def select(self, lst, loop, min_common, qid, min_score=0.0):
        if not lst:
            return []
        min_score = np.float32(min_score)
        acc_list = []
        best_acc = min_score if loop else np.float32(0)
        for si, kf in lst:
            best_score = si
            acc = si
            best_kf = kf
            for kf2 in kf.covisibles[:10]:
                if loop:
                    if not (kf2.mnLoopQuery == qid and kf2.mnLoopWords > min_common):
                        continue
                    s2 = kf2.mLoopScore
                else:
                    if kf2.mnRelocQuery != qid:
                        continue
                    s2 = kf2.mRelocScore
                acc = np.float32(acc + s2)
                if s2 > best_score:
                    best_kf = kf2
                    best_score = s2
            acc_list.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        retain = np.float32(np.float32(0.75) * best_acc)
        seen, out = set(), []
        for acc, kf in acc_list:
            if acc > retain and id(kf) not in seen:
                out.append(kf)
                seen.add(id(kf))
        return out

    def DetectLoopCandidates(self, kf, min_score):
        lst, minc, _, qid = self.query(kf.bow, True, kf.connected, min_score)
        return self.select(lst, True, minc, qid, min_score)

    def DetectRelocalizationCandidates(self, F):
        lst, minc, _, qid = self.query(F.bow, False)
        return self.select(lst, False, minc, qid)


# ------------------------------------------------------------------ test data
def random_bow(rng, n, space=512, clusters=None):
    """n distinct ascending words of [0, space) with L1-normalised positive values;
    with `clusters` (a list of word arrays) about half the words come from one of them."""
    n = min(n, space)
    words = set()
    if clusters is not None and n > 0:
        c = clusters[int(rng.integers(len(clusters)))]
        take = min(len(c), int(rng.integers(0, n // 2 + 2)), n)
        words.update(int(x) for x in rng.choice(c, take, replace=False))
    while len(words) < n:
        words.add(int(rng.integers(space)))
    w = np.array(sorted(words), np.uint32)
    v = rng.uniform(0.05, 1.0, len(w))
    if len(w):
        v = v / np.abs(v).sum()
    return w, v.astype(np.float64)
